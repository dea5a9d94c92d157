"""Sorted, tabix-indexed BGZF output on the host: the line table (svt_vcf_lines_host), the order and the gather, the writer
(bgzf_out.open_text(sort=, index=)) with deflate="zlib" and "host", the errors, and `.vcf.gz` input -- all against the checker of
tests/tbxcases.py, which shares no code with the product.  No GPU: where a driver runs, the engine seam is filled by the
oracle engine the other host tests use."""
import gzip
import io
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tbxcases as X  # noqa: E402
import test_host_pipeline as T  # noqa: E402
from svtyper_amd import bam, bgzf_out, driver, singlesample  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def as_tuples(lines):
    return [tuple(int(v) for v in row) for row in lines.tolist()]


def write(path, text, **options):
    out = bgzf_out.open_text(path, **options)
    for at in range(0, len(text), 1000):        # (in pieces, as a driver writes)
        out.write(text[at:at + 1000].decode())
    out.close()
    return open(path, "rb").read()


# ------------------------------------------------------------------------------------------ the corpus against the rule alone
@pytest.mark.parametrize("name", sorted(X.LINES))
def test_corpus_line_is_what_the_rule_says(name):
    line, (beg, end, flags) = X.LINES[name]
    got = X.parse(line)
    assert (got[0], got[1], got[3]) == (beg, end, flags)
    assert X.parse(line.rstrip(b"\n")) == got


def test_corpus_texts_are_inside_the_envelope():
    for name, text in X.TEXTS.items():
        assert X.first_out_of_order(text) is None and all(row[5] in (0, X.META) for row in X.table(text)), name
    assert len(X.TEXTS["exactly_one_payload"]) == X.PAYLOAD
    assert max(row[1] for row in X.table(X.TEXTS["spans_two_members"])) == 70000
    assert max(row[1] for row in X.table(X.TEXTS["spans_three_members"])) == 140000
    assert {name for name, text in X.ORDERS.items() if X.first_out_of_order(text)} == \
        {"reversed", "undeclared_contig", "contig_reappears", "pos_decreases", "bnd_mates_part"}


# ------------------------------------------------------------------------------------------ line table, order, gather
@pytest.mark.parametrize("name", sorted(X.TABLE_TEXTS))
def test_host_line_table_is_the_checkers(name):
    text = X.TABLE_TEXTS[name]
    assert as_tuples(nr.vcf_lines(text)) == X.table(text)


@pytest.mark.parametrize("name", sorted(X.ORDERS) + sorted(X.TEXTS))
def test_host_sort_and_gather_is_pythons_sorted(name):
    text = X.ORDERS.get(name, X.TEXTS.get(name))
    if text and not text.endswith(b"\n"):
        text += b"\n"
    lines = nr.vcf_lines(text)
    perm, bad = nr.vcf_sort_order(text, lines)
    assert bad == 0 and sorted(perm.tolist()) == list(range(len(lines)))
    assert nr.vcf_gather(text, lines, perm) == X.sorted_text(text)


def test_sort_names_a_body_line_that_is_no_data_line():
    text = X.HEADER + X.vcf_line(1, 5, "a") + X.LINES["seven_columns"][0] + X.vcf_line(1, 2, "b")
    assert nr.vcf_sort_order(text, nr.vcf_lines(text))[1] == 4
    with pytest.raises(Exception, match="no line"):
        nr.vcf_gather(text, nr.vcf_lines(text), [0, 9])


# ------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", sorted(X.TEXTS))
def test_indexed_file_answers_every_query(tmp_path, name, deflate):
    text = X.TEXTS[name]
    path = str(tmp_path / "t.vcf.gz")
    raw = write(path, text, deflate=deflate, index="tbi")
    assert gzip.decompress(raw) == text and raw.endswith(bam.BGZF_EOF)
    assert raw == write(str(tmp_path / "plain.vcf.gz"), text, deflate=deflate)        # the index changes nothing in the file
    tbi = X.read_tbi(open(path + ".tbi", "rb").read())
    members = X.Members(raw)
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(text), members)
    assert gzip.decompress(open(path + ".tbi", "rb").read()) == X.build_tbi(text, members.order)     # the fold's restatement
    if name == "no_data_lines" or name == "nothing":
        assert tbi["names"] == []


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", sorted(X.ORDERS))
def test_sorted_indexed_file(tmp_path, name, deflate):
    text = X.ORDERS[name]
    path = str(tmp_path / "s.vcf.gz")
    raw = write(path, text, deflate=deflate, huffman="dynamic" if deflate == "host" else "fixed", sort=True, index="tbi")
    want = X.sorted_text(text)
    assert gzip.decompress(raw) == want and raw.endswith(bam.BGZF_EOF)
    tbi = X.read_tbi(open(path + ".tbi", "rb").read())
    X.check_structure(raw, tbi)
    X.check_queries(raw, tbi, X.regions_of(want, n_random=50))
    assert write(str(tmp_path / "only_sorted.vcf.gz"), text, deflate=deflate, huffman="dynamic" if deflate == "host" else "fixed", sort=True) == raw
    assert not os.path.exists(str(tmp_path / "only_sorted.vcf.gz.tbi"))


def test_sort_orders_are_the_documented_ones():
    ids = lambda text: [l.split(b"\t")[2] for l in X.split_lines(text) if not l.startswith(b"#")]
    assert ids(X.sorted_text(X.ORDERS["equal_keys"])) == [b"front", b"tie0", b"tie1", b"tie2", b"tie3", b"tie4"]
    assert ids(X.sorted_text(X.ORDERS["declared_order_differs"])) == [b"b", b"a", b"c"]
    assert ids(X.sorted_text(X.ORDERS["undeclared_contig"])) == [b"b", b"a", b"z2", b"z1"]
    assert ids(X.sorted_text(X.ORDERS["pos_0_and_1"])) == [b"zero", b"one", b"one_again"]
    assert ids(X.sorted_text(X.ORDERS["bnd_mates_part"])) == [b"r_1", b"between", b"r_2"]


@pytest.mark.parametrize("name", ["reversed", "undeclared_contig", "contig_reappears", "pos_decreases", "bnd_mates_part"])
def test_unsorted_text_without_sort(tmp_path, name):
    text = X.ORDERS[name]
    path = str(tmp_path / "u.vcf.gz")
    open(path + ".tbi", "wb").write(b"an index of an earlier file")
    out = bgzf_out.open_text(path, deflate="host", index="tbi")
    out.write(text.decode())
    with pytest.raises(ValueError) as err:
        out.close()
    number = X.first_out_of_order(text)
    fields = X.split_lines(text)[number - 1].split(b"\t")
    assert isinstance(err.value, bgzf_out.VcfOrderError) and err.value.line == number
    assert "line %d" % number in str(err.value) and "%s:%s" % (fields[0].decode(), fields[1].decode()) in str(err.value)
    assert "--sort" in str(err.value)
    assert not os.path.exists(path + ".tbi")
    assert open(path, "rb").read() == write(str(tmp_path / "plain.vcf.gz"), text, deflate="host")


def test_lines_an_index_cannot_hold(tmp_path):
    for k, (line, word) in enumerate([(X.LINES["end_2_29_plus_1"][0], "CSI"), (X.LINES["seven_columns"][0], "not a VCF data line"),
                                       (X.LINES["empty"][0], "not a VCF data line"), (b"##late\n", "not a VCF data line")]):
        path = str(tmp_path / ("r%d.vcf.gz" % k))
        text = X.HEADER + X.vcf_line(1, 5, "a") + line
        out = bgzf_out.open_text(path, index="tbi")
        out.write(text.decode())
        with pytest.raises(bgzf_out.VcfOrderError, match=word) as err:
            out.close()
        assert err.value.line == 4 and not os.path.exists(path + ".tbi") and gzip.decompress(open(path, "rb").read()) == text
    out = bgzf_out.open_text(str(tmp_path / "s.vcf.gz"), sort=True)
    out.write((X.HEADER + X.LINES["pos_12a"][0]).decode())
    with pytest.raises(bgzf_out.VcfOrderError, match="line 3"):
        out.close()


def test_end_2_29_is_indexed(tmp_path):
    text = X.HEADER + X.LINES["end_2_29"][0] + X.vcf_line(1, (1 << 29) - 5, "last", ref="ACGTAC")
    raw = write(str(tmp_path / "e.vcf.gz"), text, index="tbi")
    tbi = X.read_tbi(open(str(tmp_path / "e.vcf.gz.tbi"), "rb").read())
    X.check_structure(raw, tbi)
    assert len(tbi["refs"][0]["ioff"]) == 1 << 15
    X.check_queries(raw, tbi, [(b"1", (1 << 29) - 1, 1 << 29), (b"1", 1 << 28, (1 << 28) + 1), (b"1", 0, 50), (b"1", 99, 100)])


def test_argument_errors(tmp_path):
    with pytest.raises(ValueError, match="index"):
        bgzf_out.open_text(str(tmp_path / "a.gz"), index="csi")
    with pytest.raises(ValueError, match="index_path"):
        bgzf_out.open_text(io.BytesIO(), index="tbi")
    assert not os.path.exists(str(tmp_path / "a.gz"))


def test_index_path_for_a_file_object(tmp_path):
    sink = io.BytesIO()
    kept = []
    sink.close = lambda: kept.append(sink.getvalue())
    out = bgzf_out.open_text(sink, index="tbi", index_path=str(tmp_path / "elsewhere.tbi"))
    out.write(X.TEXTS["every_indexable_line"].decode())
    out.flush()
    out.close()
    X.check_structure(kept[0], X.read_tbi(open(str(tmp_path / "elsewhere.tbi"), "rb").read()))


def cli(argv):
    import argparse
    old = sys.argv
    sys.argv = ["svtyper"] + argv
    try:
        return driver.parse_arguments(argparse.ArgumentParser(), "BAM", None, lambda p: None)
    finally:
        sys.argv = old


def test_command_line_argument_errors(tmp_path, capsys):
    for argv, word in ((["--sort"], "--bgzf"), (["--tabix", "-o", str(tmp_path / "o.vcf.gz")], "--bgzf"), (["--bgzf", "--tabix"], "output file")):
        with pytest.raises(SystemExit) as err:
            cli(["-B", "x.bam"] + argv)
        assert err.value.code != 0 and word in capsys.readouterr().err
    args = cli(["-B", "x.bam", "--bgzf", "--sort", "--tabix", "-o", str(tmp_path / "ok.vcf.gz")])
    assert args.sort and args.tabix
    args.output_vcf.close()


def test_help_does_not_list_the_options():
    import argparse
    p = argparse.ArgumentParser()
    old = sys.argv
    sys.argv = ["svtyper", "-B", "x.bam"]
    try:
        driver.parse_arguments(p, "BAM", None, lambda q: None)
    finally:
        sys.argv = old
    assert "--sort" not in p.format_help() and "--tabix" not in p.format_help()


def test_without_the_options_the_writer_is_the_old_one(tmp_path):
    text = X.TEXTS["spans_two_members"].decode()
    new, old = str(tmp_path / "new.gz"), str(tmp_path / "old.gz")
    out = bgzf_out.open_text(new, deflate="host", sort=False, index=None)
    assert out._held is None
    out.write(text)
    out.close()
    legacy = bgzf_out.BgzfTextWriter(bam.BgzfWriter(old, deflate="host"), old)
    legacy.write(text)
    legacy.close()
    assert open(new, "rb").read() == open(old, "rb").read()


# ------------------------------------------------------------------------------------------ the drivers
def run_sso(vcf_in, out):
    singlesample.sso_genotype(T.IN_BAM, vcf_in, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                              engine=T.oracle_engine, reader="python")


def no_date(data):
    return [l for l in data.split(b"\n") if not l.startswith(b"##fileDate=")]


@pytest.fixture(scope="module")
def fixture_runs(tmp_path_factory):
    """sso_genotype over the fixture: plain text, and sorted + indexed"""
    tmp = tmp_path_factory.mktemp("tbx")
    sink = io.StringIO()
    with open(T.IN_VCF) as inf:
        run_sso(inf, sink)
    path = str(tmp / "sorted.vcf.gz")
    out = bgzf_out.open_text(path, deflate="host", sort=True, index="tbi")
    with open(T.IN_VCF) as inf:
        run_sso(inf, out)
    out.close()
    return sink.getvalue().encode(), path, tmp


def contig_blocks(text):
    blocks = []
    for line in X.split_lines(text):
        if not line.startswith(b"#"):
            chrom = line.split(b"\t")[0]
            if blocks and blocks[-1][0] == chrom:
                blocks[-1][1] += 1
            else:
                blocks.append([chrom, 1])
    return [tuple(b) for b in blocks]


def test_fixture_sorted_and_indexed(fixture_runs):
    plain, path, _tmp = fixture_runs
    raw = open(path, "rb").read()
    text = gzip.decompress(raw)
    assert no_date(text) == no_date(X.sorted_text(plain)) and sorted(no_date(text)) == sorted(no_date(plain))
    assert contig_blocks(plain) == [(b"2", 113), (b"3", 97), (b"2", 1), (b"15", 1)]
    assert contig_blocks(text) == [(b"2", 114), (b"3", 97), (b"15", 1)]
    tbi = X.read_tbi(open(path + ".tbi", "rb").read())
    members = X.Members(raw)
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(text), members)


def test_fixture_without_sort_names_the_second_block(fixture_runs, tmp_path):
    plain, _path, _tmp = fixture_runs
    out = bgzf_out.open_text(str(tmp_path / "u.vcf.gz"), index="tbi")
    out.write(plain.decode())
    with pytest.raises(bgzf_out.VcfOrderError) as err:
        out.close()
    number = X.first_out_of_order(plain)
    lines = X.split_lines(plain)
    assert err.value.line == number and lines[number - 1].startswith(b"2\t") and lines[number - 2].startswith(b"3\t")
    assert not os.path.exists(str(tmp_path / "u.vcf.gz.tbi"))


def test_vcf_gz_input_gives_the_same_output(fixture_runs, tmp_path):
    plain, _path, _tmp = fixture_runs
    packed = str(tmp_path / "in.vcf.gz")
    write(packed, open(T.IN_VCF, "rb").read(), deflate="host")
    handle = open(packed)
    vcf_in = driver.gzip_text(handle)
    assert vcf_in is not handle and handle.closed
    sink = io.StringIO()
    run_sso(vcf_in, sink)
    assert no_date(sink.getvalue().encode()) == no_date(plain)
    with open(T.IN_VCF) as untouched:
        assert driver.gzip_text(untouched) is untouched
    assert driver.gzip_text(sys.stdin) is sys.stdin and driver.gzip_text(None) is None

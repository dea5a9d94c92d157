"""The CSI index of the sorted BGZF VCF without a GPU (bgzf_out.open_text(..., index="tbi", csi=True), `--csi`): the inflated
.csi against the plain-Python restatement of tests/csioutcases.py byte for byte, region queries through an independent reader
against a scan, lines beyond 2^29, the refusals, stale indexes, the argument and usage errors, and `--csi` through singlesample
over the fixture -- and the .tbi, which stays what it was."""
import argparse
import gzip
import io
import os
import struct
import sys

import pytest

import csioutcases as K
import tbxcases as X
import test_host_pipeline as T
from svtyper_amd import bam, bgzf_out, driver, singlesample
from svtyper_amd import native_reads as nr


def write(path, text, **options):
    out = bgzf_out.open_text(path, **options)
    for at in range(0, len(text), 1000):        # (in pieces, as a driver writes)
        out.write(text[at:at + 1000].decode())
    out.close()
    return open(path, "rb").read()


def read_index(path):
    raw = K.inflate(open(path, "rb").read())
    return raw, K.read_csi(raw)


FAR = X.HEADER + X.vcf_line(1, 100, "w", info="END=%d" % ((1 << 29) + 1)) + X.vcf_line(1, 5000, "inside", info="END=6000") \
    + X.vcf_line(1, 1 << 29, "at_2_29") + X.vcf_line(1, (1 << 30) + 7, "big", info="SVTYPE=DEL;END=3000000000") \
    + X.vcf_line(1, (1 << 31) - 1, "top") + X.vcf_line(2, 9, "other", info="END=%d" % ((1 << 32) - 2))
TEXTS = dict(X.TEXTS, beyond_2_29=FAR,
             end_2_29_plus_1=X.HEADER + X.vcf_line(1, 5, "a") + X.LINES["end_2_29_plus_1"][0],
             undeclared_contig=X.sorted_text(X.ORDERS["undeclared_contig"]))


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_csi_is_the_restatement_and_answers_every_query(tmp_path, name, deflate):
    text = TEXTS[name]
    path = str(tmp_path / "t.vcf.gz")
    raw = write(path, text, deflate=deflate, index="tbi", csi=True)
    assert gzip.decompress(raw) == text and raw.endswith(bam.BGZF_EOF) and not os.path.exists(path + ".tbi")
    assert raw == write(str(tmp_path / "plain.vcf.gz"), text, deflate=deflate)        # the index changes nothing in the file
    members = X.Members(raw)
    got, index = read_index(path + ".csi")
    assert got == K.build_csi_vcf(text, members.order)
    assert index["depth"] == K.vcf_depth(text) == nr.csi_depth(max([e for _c, _b, e, _l in X.data_rows(text)] or [0]))
    rows = X.data_rows(text)
    names = K.names_of(index["aux"])
    assert names == list(dict.fromkeys(r[0] for r in rows)) and len(index["refs"]) == len(names) and index["no_coor"] == 0
    for tid, ref in enumerate(index["refs"]):
        assert ref["pseudo"][1] == (sum(1 for r in rows if r[0] == names[tid]), 0)
    assert K.check_queries_vcf(index, raw) >= (200 if rows else 0)


def test_lines_beyond_2_29_index_at_depth_6(tmp_path):
    path = str(tmp_path / "far.vcf.gz")
    raw = write(path, FAR, index="tbi", csi=True)
    _bytes, index = read_index(path + ".csi")
    assert index["depth"] == 6
    m = X.Members(raw)
    ids = lambda lines: [l.split(b"\t")[2] for l in lines]
    assert ids(K.query_vcf(index, m, b"1", 2999999999, 3000000000)) == [b"big"]
    assert ids(K.query_vcf(index, m, b"1", 3000000000, 3000000001)) == []
    assert ids(K.query_vcf(index, m, b"1", 1 << 29, (1 << 29) + 1)) == [b"w"]
    assert ids(K.query_vcf(index, m, b"1", (1 << 29) - 1, 1 << 29)) == [b"w", b"at_2_29"]
    assert ids(K.query_vcf(index, m, b"2", (1 << 32) - 3, (1 << 32) - 2)) == [b"other"]
    with pytest.raises(bgzf_out.VcfOrderError, match="--csi"):         # the .tbi still refuses it, and names the way out
        write(str(tmp_path / "t.vcf.gz"), FAR, index="tbi")
    text = X.HEADER + X.LINES["end_2_29"][0]                            # an end at 2^29 exactly stays at depth 5
    write(str(tmp_path / "e.vcf.gz"), text, index="tbi", csi=True)
    assert read_index(str(tmp_path / "e.vcf.gz.csi"))[1]["depth"] == 5


def test_sorted_and_indexed(tmp_path):
    for name in sorted(X.ORDERS):
        text = X.ORDERS[name]
        path = str(tmp_path / (name + ".vcf.gz"))
        raw = write(path, text, deflate="host", huffman="dynamic", sort=True, index="tbi", csi=True)
        want = X.sorted_text(text)
        assert gzip.decompress(raw) == want
        got, index = read_index(path + ".csi")
        assert got == K.build_csi_vcf(want, X.Members(raw).order)
        K.check_queries_vcf(index, raw)


def test_refusals_leave_the_text_and_no_index(tmp_path):
    cases = [(X.LINES["end_10_digits"][0], "depth 6"), (X.LINES["seven_columns"][0], "not a VCF data line"), (b"##late\n", "not a VCF data line")]
    for k, (line, word) in enumerate(cases):
        path = str(tmp_path / ("r%d.vcf.gz" % k))
        text = X.HEADER + X.vcf_line(1, 5, "a") + line
        open(path + ".csi", "wb").write(b"an index of an earlier file")
        out = bgzf_out.open_text(path, index="tbi", csi=True)
        out.write(text.decode())
        with pytest.raises(bgzf_out.VcfOrderError, match=word) as err:
            out.close()
        assert err.value.line == 4 and not os.path.exists(path + ".csi") and gzip.decompress(open(path, "rb").read()) == text
    for name in ("reversed", "contig_reappears", "pos_decreases"):
        text = X.ORDERS[name]
        path = str(tmp_path / (name + ".vcf.gz"))
        out = bgzf_out.open_text(path, deflate="host", index="tbi", csi=True)
        out.write(text.decode())
        with pytest.raises(bgzf_out.VcfOrderError, match="--sort") as err:
            out.close()
        assert err.value.line == X.first_out_of_order(text) and ".csi index" in str(err.value) and not os.path.exists(path + ".csi")


@pytest.mark.parametrize("csi", [False, True])
def test_stale_indexes_in_either_format_are_gone(tmp_path, csi):
    path = str(tmp_path / "t.vcf.gz")
    for suffix in (".tbi", ".csi"):
        open(path + suffix, "wb").write(b"an index of an earlier file")
    write(path, X.TEXTS["every_indexable_line"], index="tbi", csi=csi)
    assert os.path.exists(path + ".csi") == csi and os.path.exists(path + ".tbi") == (not csi)


def test_argument_errors_and_index_path(tmp_path):
    with pytest.raises(ValueError, match="index"):
        bgzf_out.open_text(str(tmp_path / "a.gz"), index="csi")
    with pytest.raises(ValueError, match="csi=True"):
        bgzf_out.open_text(str(tmp_path / "a.gz"), csi=True)
    with pytest.raises(ValueError, match="csi=True"):
        bgzf_out.open_text(str(tmp_path / "a.gz"), sort=True, csi=True)
    with pytest.raises(ValueError, match="index_path"):
        bgzf_out.open_text(io.BytesIO(), index="tbi", csi=True)
    assert not os.path.exists(str(tmp_path / "a.gz"))
    text = X.TEXTS["many_short_lines"]
    raw = write(str(tmp_path / "t.vcf.gz"), text, index="tbi", csi=True, index_path=str(tmp_path / "elsewhere.csi"))
    assert not os.path.exists(str(tmp_path / "t.vcf.gz.csi"))
    assert read_index(str(tmp_path / "elsewhere.csi"))[0] == K.build_csi_vcf(text, X.Members(raw).order)


@pytest.mark.parametrize("name", ["every_indexable_line", "spans_three_members", "many_short_lines", "no_data_lines"])
def test_without_csi_the_tbi_is_what_it_was(tmp_path, name):
    text = X.TEXTS[name]
    path = str(tmp_path / "t.vcf.gz")
    raw = write(path, text, index="tbi")
    assert gzip.decompress(open(path + ".tbi", "rb").read()) == X.build_tbi(text, X.Members(raw).order)
    assert not os.path.exists(path + ".csi")


def cli(argv):
    old = sys.argv
    sys.argv = ["svtyper"] + argv
    try:
        return driver.parse_arguments(argparse.ArgumentParser(), "BAM", None, lambda p: None)
    finally:
        sys.argv = old


def test_command_line(tmp_path, capsys):
    for argv, word in ((["--csi", "-o", str(tmp_path / "o.vcf.gz")], "--csi needs --bgzf"), (["--bgzf", "--csi"], "output file"),
                       (["--bgzf", "--csi", "--tabix", "-o", str(tmp_path / "o.vcf.gz")], "--csi and --tabix")):
        with pytest.raises(SystemExit) as err:
            cli(["-B", "x.bam"] + argv)
        assert err.value.code == 2 and word in capsys.readouterr().err
    for more in ([], ["--deflate", "host", "--huffman", "dynamic"], ["--deflate", "device"], ["--deflate", "device", "--huffman", "dynamic"]):
        args = cli(["-B", "x.bam", "--bgzf", "--sort", "--csi", "-o", str(tmp_path / "ok.vcf.gz")] + more)
        assert args.sort and args.csi and not args.tabix
        args.output_vcf.close()
    p = argparse.ArgumentParser()
    old = sys.argv
    sys.argv = ["svtyper", "-B", "x.bam"]
    try:
        driver.parse_arguments(p, "BAM", None, lambda q: None)
    finally:
        sys.argv = old
    assert "--csi" not in p.format_help()


def test_csi_through_singlesample_on_the_fixture(tmp_path):
    """`svtyper-sso --bgzf --sort --csi -o PATH`: the command line's options through driver._bgzf_text, the driver over the fixture"""
    def run_sso(vcf_in, out):
        singlesample.sso_genotype(T.IN_BAM, vcf_in, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                  engine=T.oracle_engine, reader="python")
    no_date = lambda data: [l for l in data.split(b"\n") if not l.startswith(b"##fileDate=")]
    sink = io.StringIO()
    with open(T.IN_VCF) as inf:
        run_sso(inf, sink)
    path = str(tmp_path / "calls.vcf.gz")
    args = cli(["-B", T.IN_BAM, "--bgzf", "--sort", "--csi", "--deflate", "host", "-o", path])
    with driver._bgzf_text(args.output_vcf, args.deflate, 0, args.huffman, args) as out:
        with open(T.IN_VCF) as inf:
            run_sso(inf, out)
    raw = open(path, "rb").read()
    text = gzip.decompress(raw)
    assert no_date(text) == no_date(X.sorted_text(sink.getvalue().encode()))
    assert sorted(os.listdir(str(tmp_path))) == ["calls.vcf.gz", "calls.vcf.gz.csi"]
    got, index = read_index(path + ".csi")
    assert got == K.build_csi_vcf(text, X.Members(raw).order) and K.names_of(index["aux"]) == [b"2", b"3", b"15"]
    assert struct.unpack_from("<iii", got, 4)[:2] == (14, 5)
    assert K.check_queries_vcf(index, raw) > 200

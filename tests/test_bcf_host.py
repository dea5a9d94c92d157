"""BCF output on the host (svtyper_amd/csrc/svt_bcf.h through svt_bcf_encode_host; svtyper_amd/bcf_out.py; `--bcf`): the host twin
of the record rule on the corpus of tests/bcfcases.py and on the fixture's genotyped text, read back by the independent reader of
tests/bcfreader.py -- every field equals the text's field, integers and strings exactly, floats bitwise as
numpy.float32(float(token)); each refusal with its line and key; open_bcf end to end on the zlib and host deflate routes, plain
and sorted with a .csi that the independent CSI reader of tests/csioutcases.py reads; the command line's usage errors.  No GPU."""
import argparse
import io
import os
import sys

import numpy as np
import pytest

import bcfcases as X
import bcfreader as R
import csioutcases as CSI

from svtyper_amd import bcf_out, driver
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "data", "example.gt.vcf")


def check_against_text(stream, text, order=None):
    """the records of `stream` are the data lines of `text` (in `order`), the header its header; -> the records' offsets"""
    head, d, records, offsets = R.read_bcf(stream)
    lines = text.split("\n")
    body = [l for l in lines if l and not l.startswith("#")]
    assert head == "".join(l + "\n" for l in lines if l.startswith("#"))
    if order is not None:
        body = [body[i] for i in order]
    assert len(records) == len(body)
    for rec, line in zip(records, body):
        assert rec == R.line_fields(line, d), line
    return offsets


def sorted_order(text):
    """the stable (contig rank, POS) order of the data lines, restated: ranks from the ##contig lines"""
    lines = text.split("\n")
    rank = {}
    for l in lines:
        if l.startswith("##contig=<"):
            rank.setdefault(R.header_field(l, "ID"), len(rank))
    body = [l.split("\t", 2) for l in lines if l and not l.startswith("#")]
    return sorted(range(len(body)), key=lambda i: (rank[body[i][0]], int(body[i][1]), i))


@pytest.fixture(scope="module")
def corpus():
    text = X.corpus_text()
    return text, nr.bcf_encode(text.encode())


def test_dictionaries_and_header(corpus):
    text, made = corpus
    assert made["bad_line"] == 0 and made["n_ref"] == len(X.CONTIGS) and made["l_ref_max"] == X.L_REF_MAX and made["n_sample"] == len(X.SAMPLES)
    stream = made["bytes"].tobytes()
    head, d, at = R.read_header(stream)
    assert head == X.header() and at == made["header_len"]
    assert d["strings"] == X.STRINGS and d["contigs"] == X.CONTIGS and d["samples"] == list(X.SAMPLES)


def test_corpus_reads_back_field_for_field(corpus):
    text, made = corpus
    assert made["n_records"] == len(X.LINES) > 300
    offsets = check_against_text(made["bytes"].tobytes(), text)
    assert offsets == [int(o) for o in made["offsets"][:-1]] and int(made["offsets"][-1]) == made["bytes_len"]
    # the spans: what the CSI fold takes
    _head, d, records, _ = R.read_bcf(made["bytes"].tobytes())
    for rec, span, off, nxt in zip(records, made["spans"], made["offsets"][:-1], made["offsets"][1:]):
        beg = max(rec["pos"] - 1, 0)
        assert (int(span["off"]), int(span["len"]), int(span["tid"]), int(span["beg"]), int(span["end"]), int(span["flags"])) == \
            (int(off), int(nxt - off), d["contigs"].index(rec["chrom"]), beg, beg + rec["rlen"], 0)


def test_sorted_corpus(corpus):
    text, _ = corpus
    made = nr.bcf_encode(text.encode(), sort=True)
    check_against_text(made["bytes"].tobytes(), text, sorted_order(text))
    keys = made["spans"]["key"]
    assert np.all(keys[1:] >= keys[:-1])


def test_fixture_reads_back_field_for_field():
    with open(FIXTURE) as f:
        text = f.read()
    made = nr.bcf_encode(text.encode())
    assert made["bad_line"] == 0 and made["n_records"] == sum(1 for l in text.split("\n") if l and not l.startswith("#"))
    check_against_text(made["bytes"].tobytes(), text)


def test_the_devices_float_rule_is_strtod(corpus):
    """the exact rule the device uses, run on the host: the same bytes as strtod alone, and it hands over exactly the lines with
    a token outside the envelope -- none of the in-envelope corpus, none of the fixture"""
    text, made = corpus
    exact = nr.bcf_encode(text.encode(), exact_floats=True)
    assert exact["bytes"].tobytes() == made["bytes"].tobytes()
    assert exact["host_lines"] == sum(1 for _n, l in X.LINES if not X.line_in_envelope(l)) > 20
    inside = nr.bcf_encode(X.corpus_text(envelope=True).encode(), exact_floats=True)
    assert inside["host_lines"] == 0 and inside["n_records"] > 250
    with open(FIXTURE, "rb") as f:
        fixture = f.read()
    got = nr.bcf_encode(fixture, exact_floats=True)
    assert got["host_lines"] == 0 and got["bytes"].tobytes() == nr.bcf_encode(fixture)["bytes"].tobytes()


def refusal_text(line):
    good = [l for _n, l in X.LINES[:3]]
    return X.header() + "".join(l + "\n" for l in good[:2] + [line] + good[2:]), X.header().count("\n") + 3


@pytest.mark.parametrize("name,line,kind,key", X.REFUSALS, ids=[r[0] for r in X.REFUSALS])
@pytest.mark.parametrize("sort", (False, True))
def test_refusals(name, line, kind, key, sort, tmp_path):
    text, number = refusal_text(line)
    made = nr.bcf_encode(text.encode(), sort=sort)
    assert (made["bad_line"], nr.BCF_KINDS[made["bad_kind"]]) == (number, kind) and "bytes" not in made
    path = str(tmp_path / "refused.bcf")
    out = bcf_out.open_bcf(path, sort=sort, index="csi" if sort else None)
    out.write(text)
    with pytest.raises(bcf_out.BcfError) as e:
        out.close()
    assert (e.value.line, e.value.kind, e.value.key) == (number, kind, key) and "line %d" % number in str(e.value)
    assert key is None or key in str(e.value)
    with open(path, "rb") as f:
        assert f.read() == R.EOF and not os.path.exists(path + ".csi")       # as the BGZF writers leave theirs: complete, without records


def test_header_without_chrom_line_is_refused():
    with pytest.raises(Exception, match="#CHROM"):
        nr.bcf_encode(b"##fileformat=VCFv4.2\nchr1\t1\t.\tN\t.\t.\t.\t.\n")


def query(csi, mem, file_len, d, decoded, tid, beg, end):
    """the record offsets the index leads to for [beg, end) on contig `tid`; decoded: {offset: (record, next offset)}, so that a
    chunk can only be walked from a record's start"""
    ref, depth = csi["refs"][tid], csi["depth"]
    if ref["pseudo"] is None:
        return []
    floor = R.position(mem, CSI.min_offset(ref, beg, depth), file_len)
    found = set()
    for b in CSI.reg2bins(beg, min(end, 1 << (14 + 3 * depth)), depth):
        for cb, ce in ref["bins"].get(b, (0, ()))[1]:
            at, stop = R.position(mem, cb, file_len), R.position(mem, ce, file_len)
            while at < stop:
                rec, nxt = decoded[at]
                rb = max(rec["pos"] - 1, 0)                 # (POS 0, the telomere, is indexed at 0)
                if at >= floor and d["contigs"].index(rec["chrom"]) == tid and rb < end and max(rb + rec["rlen"], rb + 1) > beg:
                    found.add(at)
                at = nxt
    return sorted(found)


def check_indexed(path, text, n_ref, l_ref_max):
    with open(path, "rb") as f:
        data = f.read()
    with open(path + ".csi", "rb") as f:
        csi = CSI.read_csi(CSI.inflate(f.read()))
    mem = R.members(data)
    assert all(len(m[2]) == 65280 for m in mem[:-1])
    stream = b"".join(m[2] for m in mem)
    offsets = check_against_text(stream, text, sorted_order(text))
    _head, d, records, _ = R.read_bcf(stream)
    decoded = {at: (rec, nxt) for at, rec, nxt in zip(offsets, records, offsets[1:] + [len(stream)])}
    assert csi["depth"] == CSI.depth_for(l_ref_max) and csi["aux"] == b"" and len(csi["refs"]) == n_ref and csi["no_coor"] == 0
    # every record is found through the index, at a virtual offset the index gives
    given = {R.position(mem, v, len(data)) for ref in csi["refs"] for _l, chunks in ref["bins"].values() for c in chunks for v in c}
    rows = [(d["contigs"].index(r["chrom"]), max(r["pos"] - 1, 0), max(r["pos"] - 1, 0) + max(r["rlen"], 1)) for r in records]
    for (tid, beg, end), at in zip(rows, offsets):
        assert at in query(csi, mem, len(data), d, decoded, tid, beg, end)
    assert set(offsets) >= given - {len(stream)} and given
    # a region query returns exactly the overlapping records
    rnd = np.random.RandomState(3)
    regions = [(t, b, e) for t, b, e in rows[::7]] + [(t, max(b - 1, 0), b) for t, b, e in rows[::11]] + [(t, e, e + 1) for t, b, e in rows[::13]]
    regions += [(int(rnd.randint(n_ref)), int(lo), int(lo) + int(w)) for lo, w in zip(rnd.randint(0, 1 << 27, 60), rnd.choice([1, 1000, 1 << 17, 1 << 26], 60))]
    for tid, beg, end in regions:
        want = [at for (t, b, e), at in zip(rows, offsets) if t == tid and b < end and e > beg]
        assert query(csi, mem, len(data), d, decoded, tid, beg, end) == want, (tid, beg, end)
    return len(regions)


def indexable_text():
    """the corpus without the line at chrX:2147483646, which the scheme of these contigs (depth 5: 2^29) does not reach, and
    1 200 seeded lines behind it: several members"""
    names = [n for n, _l in X.LINES if n != "pos_top"]
    return X.corpus_text(names) + X.shaped_text(1200, 3).split("\n", X.header().count("\n"))[-1]


@pytest.mark.parametrize("deflate,huffman", (("zlib", "fixed"), ("host", "fixed"), ("host", "dynamic")))
def test_open_bcf_end_to_end(deflate, huffman, tmp_path):
    text = indexable_text()
    plain = str(tmp_path / "plain.bcf")
    with bcf_out.open_bcf(plain, deflate=deflate, huffman=huffman) as out:
        for at in range(0, len(text), 1000):            # (as the drivers write: in pieces)
            out.write(text[at:at + 1000])
    with open(plain, "rb") as f:
        stream = R.stream_of(f.read())
    assert stream == nr.bcf_encode(text.encode())["bytes"].tobytes() and len(stream) > 2 * 65280
    check_against_text(stream, text)
    indexed = str(tmp_path / "sorted.bcf")
    with open(indexed + ".csi", "wb") as f:
        f.write(b"stale")
    with bcf_out.open_bcf(indexed, deflate=deflate, huffman=huffman, sort=True, index="csi") as out:
        out.write(text)
    assert check_indexed(indexed, text, len(X.CONTIGS), X.L_REF_MAX) > 100


def test_index_of_unsorted_records_is_refused(tmp_path):
    text = X.corpus_text()
    path = str(tmp_path / "unsorted.bcf")
    with open(path + ".csi", "wb") as f:
        f.write(b"stale")
    out = bcf_out.open_bcf(path, index="csi")
    out.write(text)
    with pytest.raises(bcf_out.BcfError) as e:
        out.close()
    body = [l.split("\t") for l in text.split("\n") if l and not l.startswith("#")]
    rank = {c: i for i, c in enumerate(X.CONTIGS)}
    keys = [(rank[c[0]], max(int(c[1]) - 1, 0)) for c in body]
    first = next(i for i in range(1, len(keys)) if keys[i] < keys[i - 1]) + 1
    assert e.value.kind == "order" and e.value.line == first and "record %d" % first in str(e.value)
    assert not os.path.exists(path + ".csi")
    with open(path, "rb") as f:
        check_against_text(R.stream_of(f.read()), text)          # the BCF itself is complete


def test_open_bcf_arguments(tmp_path):
    with pytest.raises(ValueError):
        bcf_out.open_bcf(str(tmp_path / "a.bcf"), index="tbi")
    with pytest.raises(ValueError):
        bcf_out.open_bcf(io.BytesIO(), index="csi")
    with pytest.raises(ValueError):
        bcf_out.open_bcf(str(tmp_path / "b.bcf"), deflate="zlib", huffman="dynamic")


def cli(argv):
    old = sys.argv
    sys.argv = ["svtyper"] + argv
    try:
        p = argparse.ArgumentParser()
        return driver.parse_arguments(p, "BAM", None, lambda q: None), p
    finally:
        sys.argv = old


def test_command_line(tmp_path, capsys):
    o = ["-o", str(tmp_path / "o.bcf")]
    for argv, word in ((["--bcf", "--bgzf"] + o, "--bcf and --bgzf"), (["--bcf", "--tabix"] + o, "--tabix indexes VCF text"), (["--bcf", "--csi"], "output file"),
                       (["--sort"] + o, "--sort and --tabix need --bgzf"), (["--csi"] + o, "--csi needs --bgzf")):
        with pytest.raises(SystemExit) as err:
            cli(["-B", "x.bam"] + argv)
        assert err.value.code == 2 and word in capsys.readouterr().err
    for more in ([], ["--sort"], ["--sort", "--csi"], ["--deflate", "host", "--huffman", "dynamic"], ["--deflate", "device", "--sort", "--csi"]):
        args, p = cli(["-B", "x.bam", "--bcf"] + o + more)
        assert args.bcf and not args.bgzf and "--bcf" not in p.format_help()
        args.output_vcf.close()
    args, _p = cli(["-B", "x.bam"])
    assert not args.bcf


def test_bcf_through_the_drivers_writer(tmp_path):
    """what run_main hands the drivers for --bcf: the writer of open_bcf with the options of the command line"""
    args, _p = cli(["-B", "x.bam", "--bcf", "--sort", "--csi", "--deflate", "host", "-o", str(tmp_path / "cli.bcf")])
    text = indexable_text()
    with driver._bgzf_text(args.output_vcf, args.deflate, 0, args.huffman, args) as out:
        assert isinstance(out, bcf_out.BcfWriter)
        out.write(text)
    assert check_indexed(str(tmp_path / "cli.bcf"), text, len(X.CONTIGS), X.L_REF_MAX)

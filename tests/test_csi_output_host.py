"""The CSI index of the sorted `-w` BAM without a GPU (csi=True, `--alignment-csi`): the inflated .csi against the plain-Python
restatement of tests/csioutcases.py byte for byte, its depth against svt_csi_depth, structure and region queries through an
independent reader, the project's own readers over the BAM with only the .csi beside it, the refusals, stale indexes, the
argument and usage errors -- and the .bai, which stays what it was."""
import os
import struct
import sys

import numpy as np
import pytest

import baicases as B
import csioutcases as K
from svtyper_amd import bam, classic
from svtyper_amd import native_reads as nr

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
INPUTS = dict(K.all_indexable())


class Template:
    """what AlignmentFile(..., "wb", template=) reads of its template, over a header made here"""

    def __init__(self, header):
        self._header_bytes = header
        l_text = struct.unpack_from("<i", header, 4)[0]
        self.text = header[8:8 + l_text].decode("ascii")
        self.header = bam.AlignmentFile._parse_header(self.text)
        at, names, lens = 12 + l_text, [], []
        for _ in range(struct.unpack_from("<i", header, 8 + l_text)[0]):
            l_name = struct.unpack_from("<i", header, at)[0]
            names.append(header[at + 4:at + 3 + l_name].decode("ascii"))
            lens.append(struct.unpack_from("<i", header, at + 4 + l_name)[0])
            at += 8 + l_name
        self.references, self.lengths = tuple(names), tuple(lens)
        self._tid = {r: i for i, r in enumerate(names)}


def write(path, header, records, **options):
    out = bam.AlignmentFile(str(path), "wb", template=Template(header), **options)
    assert (out._held is not None) == bool(options.get("sort") or options.get("index"))
    try:
        for raw in records:
            out.write_raw(raw)
    finally:
        out.close()


def read(path):
    with open(str(path), "rb") as f:
        return f.read()


def test_writer_makes_a_csi(tmp_path):
    case = K.CASES["far"]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", csi=True)
    assert not os.path.exists(str(tmp_path / "ev.bam.bai"))
    raw = K.inflate(read(tmp_path / "ev.bam.csi"))
    assert raw[:4] == b"CSI\1" and struct.unpack_from("<iii", raw, 4) == (14, 6, 0)
    w = B.Written(read(tmp_path / "ev.bam"))
    assert max(r[3] for r in w.rows) == (1 << 32) - 2            # the record that ends at 2^32 - 2 is in the file and in the index
    assert raw == K.build_csi_bam(w)


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("label", sorted(INPUTS))
def test_csi_is_the_restatement_byte_for_byte(tmp_path, label, deflate):
    case = INPUTS[label]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", csi=True, deflate=deflate)
    w = B.Written(read(tmp_path / "ev.bam"))
    raw = K.inflate(read(tmp_path / "ev.bam.csi"))
    assert raw == K.build_csi_bam(w)
    depth = struct.unpack_from("<i", raw, 8)[0]
    assert depth == nr.csi_depth(K.l_ref_max(case.header)) == K.depth_for(K.l_ref_max(case.header))
    assert not os.path.exists(str(tmp_path / "ev.bam.bai"))
    write(tmp_path / "plain.bam", case.header, case.records, sort=True, deflate=deflate)
    assert read(tmp_path / "ev.bam") == read(tmp_path / "plain.bam")         # the BAM does not know which index it got


def test_depths_of_the_corpus_and_of_the_library():
    assert [nr.csi_depth(v) for v in (0, 1, 1 << 29, (1 << 29) + 1, 1 << 31, (1 << 32) - 1)] == [5, 5, 5, 6, 6, 6]
    assert all(nr.csi_depth(v) == K.depth_for(v) for v in (0, 1000, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, 1 << 30, (1 << 32) - 2, (1 << 32) - 1))
    depths = {K.depth_for(K.l_ref_max(case.header)) for case in INPUTS.values()}
    assert depths == {5, 6}


@pytest.mark.parametrize("label", sorted(INPUTS))
def test_structure_and_region_queries(tmp_path, label):
    case = INPUTS[label]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", csi=True)
    w = B.Written(read(tmp_path / "ev.bam"))
    index = K.read_csi(K.inflate(read(tmp_path / "ev.bam.csi")))
    K.check_structure(index, w)
    assert K.check_queries(index, w) >= 200


def test_bin_0_at_depth_6_and_the_loffset_from_the_running_maximum(tmp_path):
    case = K.CASES["bin0_depth6"]
    write(tmp_path / "a.bam", case.header, case.records, sort=True, index="bai", csi=True)
    index = K.read_csi(K.inflate(read(tmp_path / "a.bam.csi")))
    assert index["depth"] == 6 and 0 in index["refs"][0]["bins"]
    case = K.CASES["running_maximum"]
    write(tmp_path / "b.bam", case.header, case.records, sort=True, index="bai", csi=True)
    w = B.Written(read(tmp_path / "b.bam"))
    index = K.read_csi(K.inflate(read(tmp_path / "b.bam.csi")))
    first = w.voffset(w.offsets[0])                 # the long record, first in the file: it ends behind every later bin's start
    behind = [b for b, (loffset, _chunks) in index["refs"][0]["bins"].items() if K.bin_start(b, 5) > 200 and K.bin_start(b, 5) < 5000000]
    assert len(behind) > 50 and all(index["refs"][0]["bins"][b][0] == first for b in behind)


OWN_READER = ["bai:cigars", "bai:n_ref_300", "bai:three_members", "bai:long_record", "bai:member_edge", "bai:n65", "csi:far", "csi:pos_2_29_minus_1",
              "csi:end_at_depth5_limit", "csi:bin0_depth6", "csi:leaf_edges_depth5", "csi:leaf_edges_depth6", "csi:running_maximum",
              "csi:empty_references_between", "csi:long_record_depth5"]


@pytest.mark.parametrize("label", OWN_READER)
def test_own_readers_open_the_bam_with_only_the_csi(tmp_path, label):
    case = INPUTS[label]
    # (without a placed record that is flagged unmapped and has a CIGAR: the index gives it one base, the reader's own overlap
    # test measures it by its CIGAR -- tests/test_bam_sort_host.py says the same of the .bai)
    records = [raw for raw in case.records if not (struct.unpack_from("<H", raw, 18)[0] & 4 and struct.unpack_from("<H", raw, 16)[0]
                                                   and struct.unpack_from("<i", raw, 4)[0] >= 0)]
    write(tmp_path / "ev.bam", case.header, records, sort=True, index="bai", csi=True)
    assert sorted(os.listdir(str(tmp_path))) == ["ev.bam", "ev.bam.csi"]
    w = B.Written(read(tmp_path / "ev.bam"))
    want_scheme = {"kind": "csi", "min_shift": 14, "depth": K.depth_for(K.l_ref_max(case.header))}
    native = nr.NativeBam(str(tmp_path / "ev.bam"))             # svt_bam_open: the native handle takes the same index
    assert native.index_info() == want_scheme
    native.close()
    f = bam.AlignmentFile(str(tmp_path / "ev.bam"))
    try:
        assert f.index_info() == want_scheme
        placed = [r for r in w.rows if not r[4] & B.NO_COOR]
        assert f.mapped == sum(1 for r in placed if not r[4] & B.UNMAPPED)
        limit = 1 << (14 + 3 * want_scheme["depth"])
        regions = [r for r in K.regions(w, seed=3)[::7] if r[1] < min(limit, (1 << 31) - 1)]
        assert len(regions) > 30
        for tid, beg, end in regions:
            end = min(end, (1 << 31) - 1)
            got = [(r.query_name, r.flag, r.reference_start) for r in f.fetch(f.references[tid], beg, end)]
            want = []
            for at in K.scan(w, tid, beg, end):
                raw = w.records[w.offsets.index(at)]
                want.append((raw[36:36 + raw[12] - 1].decode("ascii"), struct.unpack_from("<H", raw, 18)[0], struct.unpack_from("<i", raw, 8)[0]))
            assert got == want, (tid, beg, end)
    finally:
        f.close()


def with_read_group(raw):
    """the record with its tag area replaced by RG:Z:rg1: what the native handle's fragment summariser attributes a read by"""
    l_name, n_cigar = raw[12], struct.unpack_from("<H", raw, 16)[0]
    body = raw[4:36 + l_name + 4 * n_cigar] + b"RGZrg1\0"
    return struct.pack("<i", len(body)) + body


NATIVE_FETCH = ["bai:three_members", "bai:long_record", "bai:member_edge", "csi:far", "csi:pos_2_29_minus_1", "csi:end_at_depth5_limit", "csi:bin0_depth6",
                "csi:leaf_edges_depth5", "csi:leaf_edges_depth6", "csi:running_maximum", "csi:empty_references_between", "csi:long_record_depth5"]


@pytest.mark.parametrize("label", NATIVE_FETCH)
def test_native_handle_fetches_through_the_csi(tmp_path, label):
    """svt_bam_open with only the .csi beside the BAM, svt_bam_summarise over fetch windows: every record here is a fragment of its
    own (one name each, no mate), so a window's fragments are the records the scan finds in it"""
    case = INPUTS[label]
    lens = Template(case.header).lengths
    records = [with_read_group(raw) for raw in case.records if struct.unpack_from("<i", raw, 4)[0] >= 0
               and struct.unpack_from("<i", raw, 8)[0] < lens[struct.unpack_from("<i", raw, 4)[0]]]     # (inside their contig: the reader clips a window to it)
    write(tmp_path / "ev.bam", case.header, records, sort=True, index="bai", csi=True)
    assert sorted(os.listdir(str(tmp_path))) == ["ev.bam", "ev.bam.csi"]
    w = B.Written(read(tmp_path / "ev.bam"))
    native = nr.NativeBam(str(tmp_path / "ev.bam"))
    try:
        assert native.index_info()["kind"] == "csi"
        regions = [(tid, beg, min(end, lens[tid])) for tid, beg, end in K.regions(w, seed=5)[::5] if beg < lens[tid]]
        assert len(regions) > 30
        windows = np.zeros(len(regions), nr.FETCH_DTYPE)
        for i, (tid, beg, end) in enumerate(regions):
            windows[i] = (tid, beg, end, tid, beg, end)
        off, _fragments, skipped = native.summarise(windows, np.zeros(len(regions), nr.BREAKPOINT_DTYPE), ["rg1"], [0], None, 0)
        assert not skipped.any()
        assert np.diff(off).tolist() == [len(K.scan(w, *region)) for region in regions]
    finally:
        native.close()


@pytest.mark.parametrize("deflate", ["zlib", "host"])
def test_unsorted_without_sort_is_refused_and_the_bam_is_complete(tmp_path, deflate):
    case = B.CASES["unsorted_bai_alone"]
    path = tmp_path / "ev.bam"
    with pytest.raises(bam.BamOrderError) as e:
        write(path, case.header, case.records, index="bai", csi=True, deflate=deflate)
    assert e.value.record == case.refuse[1] and "--sort-alignment" in str(e.value) and ".csi index" in str(e.value)
    assert B.Written(read(path)).records == case.records and not os.path.exists(str(path) + ".csi")


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", K.REFUSED)
def test_beyond_the_scheme_is_refused_by_record(tmp_path, name, deflate):
    case = K.CASES[name]
    number, kind = case.refuse
    path = tmp_path / "ev.bam"
    with open(str(path) + ".csi", "wb") as stale:
        stale.write(b"an earlier file's")
    with pytest.raises(bam.BamOrderError) as e:
        write(path, case.header, case.records, sort=True, index="bai", csi=True, deflate=deflate)
    raw = case.records[number - 1]
    assert e.value.record == number and kind == B.KIND_BEYOND
    assert "record %d (%s, %d:%d)" % ((number, raw[36:36 + raw[12] - 1].decode("ascii")) + struct.unpack_from("<ii", raw, 4)) in str(e.value)
    depth = K.depth_for(K.l_ref_max(case.header))
    assert "2^%d" % (14 + 3 * depth) in str(e.value) and "depth %d" % depth in str(e.value)
    assert not os.path.exists(str(path) + ".csi") and not os.path.exists(str(path) + ".bai")
    w = B.Written(read(path))                       # the BAM itself is complete and sorted
    assert w.records == [case.records[i] for i in B.order(case.records, case.n_ref)]


def test_the_bai_refusal_names_the_way_out(tmp_path):
    case = B.CASES["end_beyond_2_29"]
    with pytest.raises(bam.BamOrderError) as e:
        write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai")
    assert "CSI index is not written" in str(e.value) and "--alignment-csi" in str(e.value) and "csi=True" in str(e.value)
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", csi=True)         # ... and it is one
    index = K.read_csi(K.inflate(read(tmp_path / "ev.bam.csi")))
    K.check_structure(index, B.Written(read(tmp_path / "ev.bam")))


@pytest.mark.parametrize("csi", [False, True])
def test_stale_indexes_in_either_format_are_gone(tmp_path, csi):
    case = B.CASES["n65"]
    path = tmp_path / "ev.bam"
    for suffix in (".bai", ".csi"):
        with open(str(path) + suffix, "wb") as stale:
            stale.write(b"an earlier file's")
    write(path, case.header, case.records, sort=True, index="bai", csi=csi)
    assert os.path.exists(str(path) + ".csi") == csi and os.path.exists(str(path) + ".bai") == (not csi)
    f = bam.AlignmentFile(str(path))
    assert f.index_info()["kind"] == ("csi" if csi else "bai")
    f.close()
    # a caller's index_path: what lies there is replaced, the default paths are cleared all the same
    with open(str(path) + ".bai", "wb") as stale:
        stale.write(b"an earlier file's")
    with open(str(tmp_path / "elsewhere.csi"), "wb") as stale:
        stale.write(b"an earlier file's")
    write(path, case.header, case.records, sort=True, index="bai", csi=True, index_path=str(tmp_path / "elsewhere.csi"))
    assert K.inflate(read(tmp_path / "elsewhere.csi")) == K.build_csi_bam(B.Written(read(path)))
    assert not os.path.exists(str(path) + ".bai") and not os.path.exists(str(path) + ".csi")


def test_argument_errors(tmp_path):
    case = B.CASES["n65"]
    with pytest.raises(ValueError):
        write(tmp_path / "x.bam", case.header, case.records, index="csi")
    with pytest.raises(ValueError):
        write(tmp_path / "x.bam", case.header, case.records, index="csi", csi=True)
    with pytest.raises(ValueError, match="csi=True"):
        write(tmp_path / "x.bam", case.header, case.records, sort=True, csi=True)
    with pytest.raises(ValueError, match="csi=True"):
        write(tmp_path / "x.bam", case.header, case.records, csi=True)


@pytest.mark.parametrize("name", ["n65", "cigars", "three_members", "member_edge", "end_at_2_29"])
def test_without_csi_the_bai_is_what_it_was(tmp_path, name):
    case = B.CASES[name]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai")
    assert read(tmp_path / "ev.bam.bai") == B.build_bai(B.Written(read(tmp_path / "ev.bam")))
    assert not os.path.exists(str(tmp_path / "ev.bam.csi"))


def test_the_fold_entry_on_tables_made_here():
    """svt_csi_build_bam over a caller's table: KEY_BACK and a tid that is none, as svt_bai_build reports them"""
    rows = [(100, 50, 0 << 33 | 11 << 1, 0, 10, 20, 0), (150, 50, 0 << 33 | 6 << 1, 0, 5, 9, 0)]
    spans = np.array(rows, nr.BAM_SPAN)
    starts, offs = np.array([0, 200], np.uint64), np.array([0, 90], np.uint64)
    assert nr.csi_build_bam(spans, 1, 1000, starts, offs) == (None, 2, nr.BAM_KIND_KEY_BACK)
    assert nr.bai_build(spans, 1, starts, offs) == (None, 2, nr.BAM_KIND_KEY_BACK)
    spans = np.array([(100, 50, 3 << 33 | 11 << 1, 3, 10, 20, 0)], nr.BAM_SPAN)
    assert nr.csi_build_bam(spans, 1, 1000, np.array([0, 150], np.uint64), offs) == (None, 1, nr.BAM_KIND_TID)


def test_cli_usage_errors(monkeypatch, capsys):
    base = ["svtyper", "-B", os.path.join(DATA, "NA12878.target_loci.sorted.bam"), "-i", os.path.join(DATA, "example.vcf")]
    for more, words in ((["--alignment-csi"], "--alignment-csi needs -w"), (["-w", "x.bam", "--alignment-csi", "--bai"], "--alignment-csi and --bai"),
                        (["--csi"], "--csi needs --bgzf"), (["--bgzf", "--csi"], "--csi needs an output file"),
                        (["--bgzf", "-o", os.devnull, "--csi", "--tabix"], "--csi and --tabix")):
        monkeypatch.setattr(sys, "argv", base + more)
        with pytest.raises(SystemExit) as e:
            classic.get_args()
        assert e.value.code == 2 and words in capsys.readouterr().err
    for deflate, huffman in (("zlib", "fixed"), ("host", "dynamic"), ("device", "fixed"), ("device", "dynamic")):
        monkeypatch.setattr(sys, "argv", base + ["-w", "x.bam", "--sort-alignment", "--alignment-csi", "--deflate", deflate, "--huffman", huffman])
        args = classic.get_args()
        assert args.alignment_csi and not args.alignment_bai
    with open(os.path.join(DATA, "example.vcf")) as vcf_in, open(os.devnull, "w") as out:
        with pytest.raises(ValueError, match="need -w"):
            classic.sv_genotype(os.path.join(DATA, "NA12878.target_loci.sorted.bam"), vcf_in, out, 20, 1, 1, 1000000,
                                os.path.join(DATA, "NA12878.bam.json"), False, None, None, False, None, 1e10, alignment_index="csi")

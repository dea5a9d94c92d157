"""The coordinate-sorted, BAI-indexed `-w` BAM without a GPU: the span table and the order against the checker of
tests/baicases.py, the file-layout invariant, the .bai through structure checks and region queries, the project's own reader
over the sorted file, the refusals and the header rule."""
import os
import struct
import sys

import numpy as np
import pytest

import baicases as B
from svtyper_amd import bam, classic
from svtyper_amd import native_reads as nr


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
    # the options took effect: a writer that ignores them streams, and input that is in order already would pass for sorted
    assert (out._held is not None) == bool(options.get("sort") or options.get("index"))
    try:
        for raw in records:
            out.write_raw(raw)
    finally:
        out.close()


def read(path):
    with open(str(path), "rb") as f:
        return f.read()


def span_rows(spans):
    return [tuple(int(v) for v in row) for row in spans.tolist()]


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_spans_and_order_equal_the_checkers(name):
    case = B.CASES[name]
    data = case.header + b"".join(case.records)
    rec_off = np.cumsum([len(case.header)] + [len(r) for r in case.records]).astype(np.uint64)
    spans, key_and, key_or = nr.bam_spans(data, rec_off, case.n_ref)
    assert span_rows(spans) == B.table(len(case.header), case.records, case.n_ref)
    keys = B.keys(case.records, case.n_ref)
    want_and, want_or = 0xFFFFFFFFFFFFFFFF, 0
    for k in keys:
        want_and, want_or = want_and & k, want_or | k
    assert (key_and, key_or) == (want_and, want_or)
    perm, bad, kind = nr.bam_sort_order(spans)
    assert (bad, kind) == B.first_bad(case.records, case.n_ref)
    if case.refuse is not None and case.refuse[0] == "sort":
        assert (bad, kind) == case.refuse[1:] and perm is None
    else:
        assert perm.tolist() == B.order(case.records, case.n_ref)


def test_the_two_sorting_inputs_on_the_host():
    for case in (B.single_pass_case(), B.every_digit_case()):
        rec_off = np.cumsum([0] + [len(r) for r in case.records]).astype(np.uint64)
        spans, key_and, key_or = nr.bam_spans(b"".join(case.records), rec_off, case.n_ref)
        assert span_rows(spans) == B.table(0, case.records, case.n_ref)
        differ = key_and ^ key_or
        digits = sum(1 for d in range(8) if differ >> (8 * d) & 255)
        assert digits == (1 if case.n_ref == 1 else 8)
        assert nr.bam_sort_order(spans)[0].tolist() == B.order(case.records, case.n_ref)


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", B.SORTABLE)
def test_sorted_file_is_the_file_of_sorted_records(tmp_path, name, deflate):
    case = B.CASES[name]
    write(tmp_path / "sorted.bam", case.header, case.records, sort=True, deflate=deflate)
    in_order = [case.records[i] for i in B.order(case.records, case.n_ref)]
    write(tmp_path / "plain.bam", B.coordinate_header(case.header), in_order, deflate=deflate)
    got = read(tmp_path / "sorted.bam")
    assert got == read(tmp_path / "plain.bam")
    w = B.Written(got)
    assert w.records == in_order and w.header == B.coordinate_header(case.header)
    assert [p for _off, p in w.members] == B.payloads(w.header, in_order)
    assert not os.path.exists(str(tmp_path / "sorted.bam.bai"))


def test_dynamic_blocks_keep_the_layout(tmp_path):
    case = B.CASES["three_members"]
    write(tmp_path / "sorted.bam", case.header, case.records, sort=True, index="bai", deflate="host", huffman="dynamic")
    in_order = [case.records[i] for i in B.order(case.records, case.n_ref)]
    write(tmp_path / "plain.bam", B.coordinate_header(case.header), in_order, deflate="host", huffman="dynamic")
    assert read(tmp_path / "sorted.bam") == read(tmp_path / "plain.bam")
    w = B.Written(read(tmp_path / "sorted.bam"))
    assert len(w.members) >= 4                      # the header's and at least three of records
    assert read(tmp_path / "sorted.bam.bai") == B.build_bai(w)


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", ["member_edge", "member_edge_last"])
def test_whole_records_fill_a_member_to_its_last_byte(tmp_path, name, deflate):
    case = B.CASES[name]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", deflate=deflate)
    w = B.Written(read(tmp_path / "ev.bam"))
    record_ends = {at + len(raw) for at, raw in zip(w.offsets, w.records)}
    full = [k for k, (_off, p) in enumerate(w.members) if k and len(p) == B.PAYLOAD]
    assert len(full) == 1
    k = full[0]
    assert w.starts[k] in w.offsets and w.starts[k] + B.PAYLOAD in record_ends          # ten whole records, none cut
    assert w.stream[w.starts[k]:w.starts[k] + B.PAYLOAD] == b"".join(w.records[:10])
    assert (k == len(w.members) - 1) == (name == "member_edge_last")
    index = B.read_bai(read(tmp_path / "ev.bam.bai"))
    B.check_structure(index, w)
    # the tenth record ends on the member's last byte: its chunk ends at the next member's first, or where the members end
    last, _counts = index["refs"][0]["pseudo"]
    end = last[1]
    assert end & 0xFFFF == 0 and w.position(end) == w.starts[k] + B.PAYLOAD
    assert (end >> 16 == w.end_of_members) == (name == "member_edge_last")
    assert read(tmp_path / "ev.bam.bai") == B.build_bai(w)


@pytest.mark.parametrize("name", B.INDEXABLE)
def test_bai_structure_and_region_queries(tmp_path, name):
    case = B.CASES[name]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai")
    w = B.Written(read(tmp_path / "ev.bam"))
    data = read(tmp_path / "ev.bam.bai")
    index = B.read_bai(data)
    B.check_structure(index, w)
    assert B.check_queries(index, w) >= 200
    assert data == B.build_bai(w)                   # the checker's own fold of the same file: the same rule, the same bytes


@pytest.mark.parametrize("name", ["cigars", "n_ref_300", "three_members", "long_record", "member_edge", "member_edge_last", "end_at_2_29", "n65"])
def test_own_reader_fetches_through_the_index(tmp_path, name):
    case = B.CASES[name]
    # (without the placed record that is flagged unmapped and has a CIGAR: the index gives it one base, the reader's own overlap
    # test measures it by its CIGAR as pysam's reference_end does -- the two answer differently by design, not through the index)
    records = [raw for raw in case.records if not (struct.unpack_from("<H", raw, 18)[0] & 4 and struct.unpack_from("<H", raw, 16)[0]
                                                   and struct.unpack_from("<i", raw, 4)[0] >= 0)]
    write(tmp_path / "ev.bam", case.header, records, sort=True, index="bai")
    w = B.Written(read(tmp_path / "ev.bam"))
    f = bam.AlignmentFile(str(tmp_path / "ev.bam"))
    try:
        assert f.index_info()["kind"] == "bai"
        placed = [r for r in w.rows if not r[4] & B.NO_COOR]
        unmapped_placed = sum(1 for r in placed if r[4] & B.UNMAPPED)
        assert f.mapped == len(placed) - unmapped_placed
        assert f.unmapped == unmapped_placed + sum(1 for r in w.rows if r[4] & B.NO_COOR)
        regions = B.regions(w, seed=3)[::7]
        assert len(regions) > 30
        for tid, beg, end in regions:
            got = [(r.query_name, r.flag, r.reference_start) for r in f.fetch(f.references[tid], beg, end)]
            want = []
            for at in B.scan(w, tid, beg, end):
                raw = w.records[w.offsets.index(at)]
                want.append((raw[36:36 + raw[12] - 1].decode("ascii"), struct.unpack_from("<H", raw, 18)[0], struct.unpack_from("<i", raw, 8)[0]))
            assert got == want, (tid, beg, end)
    finally:
        f.close()


REFUSALS = sorted(name for name, case in B.CASES.items() if case.refuse is not None)


@pytest.mark.parametrize("deflate", ["zlib", "host"])
@pytest.mark.parametrize("name", REFUSALS)
def test_refusals_name_the_record_and_leave_no_index(tmp_path, name, deflate):
    case = B.CASES[name]
    when, number, kind = case.refuse
    path = tmp_path / "ev.bam"
    with open(str(path) + ".bai", "wb") as stale:
        stale.write(b"BAI\1 of an earlier file")
    options = dict(index="bai", deflate=deflate) if when == "order" else dict(sort=True, index="bai", deflate=deflate)
    with pytest.raises(bam.BamOrderError) as e:
        write(path, case.header, case.records, **options)
    assert isinstance(e.value, ValueError) and e.value.record == number
    raw = case.records[number - 1]
    name_of = raw[36:36 + raw[12] - 1].decode("ascii")
    assert "record %d (%s, %d:%d)" % ((number, name_of) + struct.unpack_from("<ii", raw, 4)) in str(e.value)
    assert not os.path.exists(str(path) + ".bai")
    if kind == B.KIND_BEYOND:
        assert "CSI index is not written" in str(e.value)
    if when in ("index", "order"):                  # the BAM itself is complete
        w = B.Written(read(path))
        want = case.records if when == "order" else [case.records[i] for i in B.order(case.records, case.n_ref)]
        assert w.records == want
    if when == "order":
        assert "--sort-alignment" in str(e.value)
        assert B.Written(read(path)).header == case.header      # written as always: the header untouched
    if when == "sort":                              # sorting alone refuses it as well
        with pytest.raises(bam.BamOrderError) as e2:
            write(tmp_path / "s.bam", case.header, case.records, sort=True, deflate=deflate)
        assert e2.value.record == number
    if when == "index":                             # ... and sorts this one
        write(tmp_path / "s.bam", case.header, case.records, sort=True, deflate=deflate)
        assert len(B.Written(read(tmp_path / "s.bam")).records) == len(case.records)


@pytest.mark.parametrize("head", sorted(B.HEADERS))
def test_header_rule(tmp_path, head):
    case = B.CASES["header_" + head]
    write(tmp_path / "sorted.bam", case.header, case.records, sort=True)
    w = B.Written(read(tmp_path / "sorted.bam"))
    assert w.text == B.WANT_HEADERS[head] and w.header == B.coordinate_header(case.header)
    assert w.header[8 + len(w.text):] == case.header[8 + len(B.HEADERS[head]):]     # the references byte for byte
    if head == "so_coordinate":
        assert w.header == case.header
    write(tmp_path / "plain.bam", case.header, case.records)
    assert B.Written(read(tmp_path / "plain.bam")).header == case.header
    write(tmp_path / "indexed.bam", case.header, [case.records[i] for i in B.order(case.records, case.n_ref)], index="bai")
    assert B.Written(read(tmp_path / "indexed.bam")).header == case.header


def test_without_the_options_the_writer_streams_as_before(tmp_path):
    case = B.CASES["three_members"]
    out = bam.AlignmentFile(str(tmp_path / "plain.bam"), "wb", template=Template(case.header))
    assert out._held is None
    out.write_raw(case.records[0])
    out._writer._f.flush()
    assert os.path.getsize(str(tmp_path / "plain.bam")) > 0       # the header's member is in the file before close()
    for raw in case.records[1:]:
        out.write_raw(raw)
    out.close()
    w = B.Written(read(tmp_path / "plain.bam"))
    assert w.records == case.records and [p for _off, p in w.members] == B.payloads(case.header, case.records)
    assert not os.path.exists(str(tmp_path / "plain.bam.bai"))


def test_index_path_and_bad_index_value(tmp_path):
    case = B.CASES["n65"]
    write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", index_path=str(tmp_path / "elsewhere.bai"))
    assert not os.path.exists(str(tmp_path / "ev.bam.bai"))
    assert read(tmp_path / "elsewhere.bai") == B.build_bai(B.Written(read(tmp_path / "ev.bam")))
    with pytest.raises(ValueError):
        write(tmp_path / "x.bam", case.header, case.records, index="csi")


def test_options_need_write_alignment(monkeypatch, capsys):
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
    for option in ("--sort-alignment", "--bai"):
        monkeypatch.setattr(sys, "argv", ["svtyper", "-B", os.path.join(data, "NA12878.target_loci.sorted.bam"), "-i",
                                          os.path.join(data, "example.vcf"), option])
        with pytest.raises(SystemExit) as e:
            classic.get_args()
        assert e.value.code == 2 and "--sort-alignment and --bai need -w" in capsys.readouterr().err
    for options in (dict(alignment_sort=True), dict(alignment_index="bai")):
        with open(os.path.join(data, "example.vcf")) as vcf_in, open(os.devnull, "w") as out:
            with pytest.raises(ValueError, match="need -w"):
                classic.sv_genotype(os.path.join(data, "NA12878.target_loci.sorted.bam"), vcf_in, out, 20, 1, 1, 1000000,
                                    os.path.join(data, "NA12878.bam.json"), False, None, None, False, None, 1e10, **options)

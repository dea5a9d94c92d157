"""svtyper_amd/cram.py and the native slice decoder (svt_cram.h) against CRAM files written by tests/cramwriter.py, an independent
writer made from the same published text: every record read back equals the BAM record it was written from, in every layout
the reader has to take; the fetches of the fixture's breakpoints give what the BAM's give; every damaged variant is refused
with one CramError.  Host only: the rANS blocks go through the host twin."""
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramcases as cc  # noqa: E402
import cramwriter as cw  # noqa: E402
from svtyper_amd import bam, cram  # noqa: E402


class _Refs:
    """what an AlignedSegment asks of its file"""
    references = ()


def rg_first(tag_bytes, rg_ids):
    """the tag area with the RG:Z of a read group of the header in front: where the format's readers put it"""
    tags = cw.split_tags(tag_bytes)
    for t in tags:
        if t[0] == b"RGZ" and t[1][:-1].decode() in rg_ids:
            tags.remove(t)
            tags.insert(0, t)
            break
    return b"".join(k + v for k, v in tags)


def fields(r, name=None, rg_ids=()):
    return (r.query_name if name is None else name, r.flag, r.reference_id, r.reference_start, r.mapping_quality, r.cigar,
            r.next_reference_id, r.next_reference_start, r.template_length, rg_first(r._tagbytes, rg_ids), r.query_length)


def all_bam_records(path):
    """(header text, every record of the BAM without its block_size, the unplaced included)"""
    f = bam.AlignmentFile(path)
    out = []
    f._bgzf.seek(f._first_record)
    while True:
        r = f._next_record()
        if r is None:
            break
        out.append(r._raw)
    text = f.text
    f.close()
    return text, out


def rg_ids_of(text):
    return [f[3:] for line in text.splitlines() if line.startswith("@RG") for f in line.split("\t") if f.startswith("ID:")]


def read_back(path):
    """every record of the CRAM, the unplaced included"""
    f = cram.CramFile(path, verify=True)
    out = list(f._walk())
    return f, out


def check_file(path, text, records, layout):
    info = cw.write_cram(path, text, records, layout)
    f, got = read_back(path)
    rg_ids = rg_ids_of(text)
    assert len(got) == len(records)
    for k, (raw, r) in enumerate(zip(records, got)):
        want = bam.AlignedSegment(_Refs, raw)
        assert fields(r, rg_ids=rg_ids) == fields(want, info["names"][k].decode(), rg_ids), (k, want.query_name)
        # what the decoder makes up: SEQ `N`, QUAL 0xFF, the bin of the record's extent
        l_name, n_cigar, l_seq = r._raw[8], struct.unpack_from("<H", r._raw, 12)[0], r.query_length
        at = 32 + l_name + 4 * n_cigar
        assert r._raw[at:at + (l_seq + 1) // 2] == (b"\xff" * (l_seq // 2) + (b"\xf0" if l_seq & 1 else b""))
        assert r._raw[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq] == b"\xff" * l_seq
        assert struct.unpack_from("<H", r._raw, 10)[0] == struct.unpack_from("<H", raw, 10)[0], "bin"
    return f, got, info


@pytest.mark.parametrize("name,layout", cc.layouts(), ids=[n for n, _ in cc.layouts()])
def test_every_layout_reads_back(tmp_path, name, layout):
    records = cc.mixed_records()
    f, got, info = check_file(str(tmp_path / "mixed.cram"), cc.HEADER, records, layout)
    placed = [r for r in got if r.reference_id >= 0]
    assert [x.query_name for x in f.fetch()] == [x.query_name for x in placed]
    assert f.mapped == sum(1 for r in got if not r.flag & 4) and f.unmapped == sum(1 for r in got if r.flag & 4)
    assert f.count() == len(placed) and f.count(read_callback="all") == sum(1 for r in placed if not r.flag & 0x704)
    assert f.references == ("chr1", "chr2") and f.lengths == (100000, 5000) and f.gettid("chr2") == 1 and f.gettid("nope") == -1
    assert [rg["ID"] for rg in f.header["RG"]] == ["rg1", "rg2"] and f.filename.endswith("mixed.cram")
    # fetch against a scan of the records, at the slice borders too
    for contig, beg, end in (("chr1", 0, 100000), ("chr1", 99999, 100000), ("chr1", 500, 501), ("chr1", 1003, 1019), ("chr1", 1128, 1140),
                             ("chr2", 1199, 1201), ("chr2", 0, 250), ("chr2", 1100, 1400), ("chr1", 5000, 90000)):
        tid = f.gettid(contig)
        want = [r.query_name + "/%d" % r.flag for r in placed if r.reference_id == tid and r.reference_start < end
                and max(r.reference_end or 0, r.reference_start + 1) > beg]
        assert [r.query_name + "/%d" % r.flag for r in f.fetch(contig, beg, end)] == want, (contig, beg, end)
    with pytest.raises(ValueError):
        list(f.fetch("nope", 0, 10))
    f.close()


def test_names_that_are_made_up_are_shared_by_mates_and_unique(tmp_path):
    records = cc.mixed_records()
    path = str(tmp_path / "n.cram")
    cw.write_cram(path, cc.HEADER, records, cw.Layout(names=False, records_per_slice=1000))
    f, got = read_back(path)
    by_source = {}
    for raw, r in zip(records, got):
        by_source.setdefault(bam.AlignedSegment(_Refs, raw).query_name, set()).add(r.query_name)
    assert all(len(v) == 1 for v in by_source.values())                       # mates share their name
    assert len({next(iter(v)) for v in by_source.values()}) == len(by_source)   # and no two templates do
    f.close()


def test_three_hundred_read_groups(tmp_path):
    header, records = cc.many_groups()
    f, got, _ = check_file(str(tmp_path / "rg.cram"), header, records, cw.default_layout(records_per_slice=64))
    assert got[7].get_tag("RG") == "g049"
    f.close()


@pytest.fixture(scope="module")
def fixture_cram(tmp_path_factory):
    text, records = all_bam_records(cc.FIXTURE_BAM)
    path = str(tmp_path_factory.mktemp("cram") / "fixture.cram")
    info = cw.write_cram(path, text, records, cw.default_layout())
    return path, text, records, info


def test_the_fixture_reads_back(fixture_cram):
    path, text, records, info = fixture_cram
    f, got = read_back(path)
    rg_ids = rg_ids_of(text)
    assert len(got) == len(records) and len(info["slices"]) > 1
    for k, (raw, r) in enumerate(zip(records, got)):
        assert fields(r, rg_ids=rg_ids) == fields(bam.AlignedSegment(_Refs, raw), rg_ids=rg_ids), k
    b = bam.AlignmentFile(cc.FIXTURE_BAM)
    assert (f.mapped, f.unmapped) == (b.mapped, b.unmapped)
    assert f.count() == b.count() and f.count(read_callback="all") == b.count(read_callback="all")
    assert f.references == b.references and f.lengths == b.lengths and f.header == b.header
    f.close()
    b.close()


def test_fixture_fetches_of_the_golden_breakpoints_and_of_the_borders(fixture_cram):
    path, text, records, info = fixture_cram
    f, b = cram.CramFile(path), bam.AlignmentFile(cc.FIXTURE_BAM)
    regions = []
    with open(os.path.join(cc.DATA, "example.gt.vcf")) as vcf:
        for line in vcf:
            if line.startswith("#"):
                continue
            v = line.split("\t")
            pos = int(v[1])
            info_f = dict(x.split("=", 1) for x in v[7].split(";") if "=" in x)
            regions.append((v[0], max(pos - 1000, 0), pos + 1000))
            if "END" in info_f:
                regions.append((info_f.get("CHR2", v[0]), max(int(info_f["END"]) - 1000, 0), int(info_f["END"]) + 1000))
    # regions that straddle slice and container borders: around the first record of every slice
    at = 0
    for _coff, _lm, n in info["slices"]:
        first = bam.AlignedSegment(_Refs, records[at])
        if first.reference_id >= 0:
            name = b.references[first.reference_id]
            regions += [(name, max(first.reference_start - 50, 0), first.reference_start + 50), (name, first.reference_start, first.reference_start + 1)]
        at += n
    assert len(regions) > 20
    key = lambda r: (r.query_name, r.flag, r.reference_start, r.cigar, r.template_length)      # noqa: E731
    some = 0
    for contig, beg, end in regions:
        if b.gettid(contig) < 0:
            continue
        want = [key(r) for r in b.fetch(contig, beg, end)]
        assert [key(r) for r in f.fetch(contig, beg, end)] == want, (contig, beg, end)
        assert f.count(contig, beg, end, read_callback="all") == b.count(contig, beg, end, read_callback="all")
        some += len(want)
    assert some > 0 and len(f._cache) <= cram.SLICE_CACHE
    f.close()
    b.close()


@pytest.mark.parametrize("knob,says", cc.DAMAGED, ids=[k for k, _ in cc.DAMAGED])
def test_damaged_files_are_refused(tmp_path, knob, says):
    path = str(tmp_path / "damaged.cram")
    cw.write_cram(path, cc.HEADER, cc.mixed_records(), cw.default_layout(records_per_slice=20, damage=knob))
    with pytest.raises(cram.CramError) as e:
        f = cram.CramFile(path, verify=True)
        list(f._walk())
    assert says in str(e.value) and path in str(e.value)
    assert len(str(e.value).splitlines()) == 1


def test_index_names_and_the_error_without_one(tmp_path):
    path = str(tmp_path / "s.cram")
    cw.write_cram(path, cc.HEADER, cc.mixed_records(), cw.Layout())
    want = [r.query_name for r in cram.CramFile(path).fetch("chr2", 0, 5000)]
    os.rename(path + ".crai", str(tmp_path / "s.crai"))                  # sample.crai is looked for second
    assert [r.query_name for r in cram.CramFile(path).fetch("chr2", 0, 5000)] == want and want
    os.remove(str(tmp_path / "s.crai"))
    with pytest.raises(ValueError) as e:
        list(cram.CramFile(path).fetch("chr2", 0, 5000))
    assert "s.cram.crai" in str(e.value) and "s.crai" in str(e.value).replace("s.cram.crai", "")
    assert cram.is_cram(path) and not cram.is_cram(cc.FIXTURE_BAM)

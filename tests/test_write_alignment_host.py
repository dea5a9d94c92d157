"""`svtyper -w` on the host: the BAM writer (svtyper_amd/bam.py), and classic.sv_genotype(..., alignment_outpath=...) against what
the reference's own -w code handed to its output BAM (tests/golden/write_alignment.json.gz, made by
tests/golden/make_golden_write_alignment.py with a recording stand-in for pysam's writer).

No GPU here: the engine seam is filled by verdictcases.VerdictOracleEngine -- the C oracle for the result records, the Python
restatement of the six verdict bits for what the device answers (tests/test_verdicts_device.py compares the kernel with that
restatement byte for byte; tests/test_write_alignment_device.py runs these cases through the HIP engine)."""
import gzip
import io
import os
import struct
import sys
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_host_pipeline as T  # noqa: E402
import verdictcases as V  # noqa: E402
from svtyper_amd import bam, classic, sharded  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return V.golden_cases()


def no_date(text):
    return [l for l in text.split("\n") if not l.startswith("##fileDate=")]


def run_w(bams, vcf_path, lib_json, out_bam, sum_quals=False, max_reads=None, engine=None, **kw):
    """sv_genotype with -w; returns the VCF lines without ##fileDate"""
    out = io.StringIO()
    out.close = lambda: None
    with open(vcf_path) as inf:
        classic.sv_genotype(bams, inf, out, 20, 1, 1, 1000000, lib_json, False, out_bam, None, sum_quals, max_reads, 1e10,
                            engine=engine or V.VerdictOracleEngine(), **kw)
    return no_date(out.getvalue())


def same_writes(path, case):
    writes, mapq = V.written_records(path)
    assert len(writes) == len(case["writes"])
    for i, (got, want) in enumerate(zip(writes, case["writes"])):
        assert got == want, "record %d" % i
    assert mapq == case["mapq"]


# ------------------------------------------------------------------------------------------ the writer
def members(path):
    """(offset, size, payload size) of every BGZF member of a file, walked by BSIZE"""
    data = open(path, "rb").read()
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        payload = zlib.decompress(data[at + 18:at + size - 8], -15)
        assert len(payload) == isize and zlib.crc32(payload) & 0xFFFFFFFF == crc
        out.append((at, size, isize))
        at += size
    assert at == len(data)
    return out


def all_records(path):
    f = bam.AlignmentFile(path, "rb", verify=True)
    f._bgzf.seek(f._first_record)
    out = []
    while True:
        r = f._next_record()
        if r is None:
            break
        out.append(r)
    return f, out


def tag_fields(b):
    """[(name, the field's bytes)] of a tag area whose values are of the types the fixture uses"""
    out, i = [], 0
    while i < len(b):
        t = chr(b[i + 2])
        j = b.index(b"\0", i + 3) + 1 if t in "ZH" else i + 3 + {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[t]
        out.append((b[i:i + 2], b[i:j]))
        i = j
    return out


def without_xv(b):
    return b"".join(field for name, field in tag_fields(b) if name != b"XV")


def test_writer_round_trip(tmp_path):
    """The fixture's own reads: most carry an XV:Z tag (the file is itself such a dump), some carry none -- so XV is replaced
    where it is present and appended where it is absent.  Every fifth tagged read also gets an XW:i behind its XV, so that the
    second pass replaces an XV in the middle of a tag area."""
    src = bam.AlignmentFile(T.IN_BAM, "rb")
    src._bgzf.seek(src._first_record)
    reads = [src._next_record() for _ in range(6000)]
    assert all(r is not None for r in reads)
    had_xv = [b"XV" in [name for name, _ in tag_fields(r._tagbytes)] for r in reads]
    want_xv = [("R", "A", None)[i % 3] for i in range(len(reads))]
    assert {(h, x) for h, x in zip(had_xv, want_xv)} == {(h, x) for h in (True, False) for x in ("R", "A", None)}
    first = str(tmp_path / "first.bam")
    out = bam.AlignmentFile(first, "wb", template=src)
    for i, (r, xv) in enumerate(zip(reads, want_xv)):
        if xv is not None:
            r.set_tag("XV", xv)
            if i % 5 == 0:
                r.set_tag("XW", i)
        r.query_sequence = None
        out.write(r)
    out.close()

    ms = members(first)
    assert len(ms) > 3                                             # header, several members of records, EOF
    assert all(size <= 0x10000 and isize <= 0x10000 for _, size, isize in ms)
    assert open(first, "rb").read()[-28:] == bam.BGZF_EOF and ms[-1][2] == 0
    back_file, back = all_records(first)                            # verify="crc32": every member's CRC32 is checked
    assert back_file.text == src.text and back_file._header_bytes == src._header_bytes
    assert back_file.references == src.references and back_file.lengths == src.lengths
    assert len(back) == len(reads)
    for i, (r, b, xv) in enumerate(zip(reads, back, want_xv)):
        for name in ("reference_id", "reference_start", "mapping_quality", "flag", "next_reference_id", "next_reference_start",
                     "template_length", "query_name", "cigar"):
            assert getattr(b, name) == getattr(r, name), name
        assert b._raw[10:12] == r._raw[10:12]                       # bin: the original's
        assert b.query_length == 0 and struct.unpack_from("<i", b._raw, 16)[0] == 0      # l_seq = 0, no sequence, no qualities
        if xv is None:                                              # not set: the tag area as it was
            assert b._tagbytes == r._tagbytes
        else:                                                       # as type A, behind the other tags, which keep their order
            xw = b"XWi" + struct.pack("<i", i) if i % 5 == 0 else b""
            assert b._tagbytes == without_xv(r._tagbytes) + b"XVA" + xv.encode() + xw and b.get_tag("XV") == xv
    assert back_file._bgzf.members_verified >= len(ms) - 1

    # XV present in the record: replaced, not added a second time
    second = str(tmp_path / "second.bam")
    out = bam.AlignmentFile(second, "wb", template=back_file)
    flipped = {"R": "A", "A": "R"}
    before = [b._tagbytes for b in back]
    assert any(not t.endswith(b"XVA" + xv.encode()) for t, xv in zip(before, want_xv) if xv is not None)      # (the XW reads)
    for b, xv in zip(back, want_xv):
        if xv is not None:
            b.set_tag("XV", flipped[xv])
        out.write(b)
    out.close()
    again_file, again = all_records(second)
    assert again_file._header_bytes == src._header_bytes
    for t, a, xv in zip(before, again, want_xv):
        if xv is None:
            assert a._tagbytes == t
        else:
            assert a._tagbytes == without_xv(t) + b"XVA" + flipped[xv].encode()
            assert [name for name, _ in tag_fields(a._tagbytes)].count(b"XV") == 1
    for f in (src, back_file, again_file):
        f.close()


def test_writer_keeps_a_large_record_whole_and_members_small(tmp_path):
    """a tag area of 200 KB: the record spans members of at most 64 KiB each and reads back the same"""
    src = bam.AlignmentFile(T.IN_BAM, "rb")
    src._bgzf.seek(src._first_record)
    r = src._next_record()
    r.set_tag("XL", "".join(chr(33 + (i * 7) % 90) for i in range(200000)))
    path = str(tmp_path / "large.bam")
    out = bam.AlignmentFile(path, "wb", template=src)
    out.write(r)
    out.close()
    assert all(size <= 0x10000 and isize <= 0x10000 for _, size, isize in members(path))
    f, (b,) = all_records(path)
    assert b.get_tag("XL") == r.get_tag("XL") and b.query_name == r.query_name
    f.close()
    src.close()


# ------------------------------------------------------------------------------------------ the golden's reach
def test_golden_reach(golden):
    a = golden["a"]
    tags = [w[4] for w in a["writes"]]
    assert (len(tags), tags.count("R"), tags.count("A"), tags.count(None)) == (42799, 32977, 8065, 1757)
    for case in golden.values():
        keys = [(w[0], w[1]) for w in case["writes"]]
        assert len(set(keys)) == len(keys)                          # a (name, flag) is written once
        assert {w[4] for w in case["writes"]} == {"R", "A", None}
        # a read with MAPQ 0 tagged R: the 16-byte record cannot show its is_ref_seq hit (its gated MAPQ byte is 0 either way)
        assert any(q == 0 and w[4] == "R" for w, q in zip(case["writes"], case["mapq"]))
    # the fixture given twice: every read of the first sample's units comes again in the second sample's and is written once
    assert golden["twice"]["writes"] == a["writes"] and golden["twice"]["mapq"] == a["mapq"]


# ------------------------------------------------------------------------------------------ sv_genotype(..., alignment_outpath=...)
def test_fixture_case_a(tmp_path, golden):
    out_bam = str(tmp_path / "a.bam")
    vcf = run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam)
    assert vcf == no_date(open(T.EXPECTED).read())
    same_writes(out_bam, golden["a"])
    f = bam.AlignmentFile(out_bam, "rb")
    t = bam.AlignmentFile(T.IN_BAM, "rb")
    assert f._header_bytes == t._header_bytes                       # the first -B file is the template
    f.close()
    t.close()


def test_fixture_twice_the_written_set_is_the_runs(tmp_path, golden):
    out_bam = str(tmp_path / "twice.bam")
    vcf = run_w(T.IN_BAM + "," + T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam, sum_quals=True)
    assert vcf == gzip.open(os.path.join(HERE, "golden", "example.twice.sumquals.gt.vcf.gz"), "rt").read().split("\n")
    same_writes(out_bam, golden["twice"])


def test_three_samples_blank_in_the_middle(tmp_path, golden):
    from test_multisample_qual import three_sample_case
    bams, vcf_path, lib_json = three_sample_case(str(tmp_path))
    out_bam = str(tmp_path / "three_w.bam")
    vcf = run_w(bams, vcf_path, lib_json, out_bam)
    assert vcf == gzip.open(os.path.join(HERE, "golden", "three.gt.vcf.gz"), "rt").read().split("\n")
    same_writes(out_bam, golden["three"])


def test_three_samples_in_several_library_groups(tmp_path, golden, monkeypatch):
    """one device batch per sample (pipeline.library_groups): the verdicts of every group's batch go back to its units"""
    from svtyper_amd import pipeline
    from test_multisample_qual import three_sample_case
    monkeypatch.setattr(pipeline, "MAX_BATCH_LIBS", 2)      # (two libraries per sample)
    calls = []

    class Counting(V.VerdictOracleEngine):
        def __call__(self, batch, flags=0, verdicts=False):
            calls.append(batch.n_units)
            return super().__call__(batch, flags, verdicts=verdicts)
    bams, vcf_path, lib_json = three_sample_case(str(tmp_path))
    out_bam = str(tmp_path / "three_groups.bam")
    vcf = run_w(bams, vcf_path, lib_json, out_bam, engine=Counting())
    assert len(calls) == 3
    assert vcf == gzip.open(os.path.join(HERE, "golden", "three.gt.vcf.gz"), "rt").read().split("\n")
    same_writes(out_bam, golden["three"])


def test_small_chunks_write_the_same_bam(tmp_path, golden, monkeypatch):
    """a flush every 7 units: the (name, flag) set and the write order hold across chunks in flight (ChunkPipeline)"""
    from svtyper_amd import driver
    from test_multisample_qual import three_sample_case
    monkeypatch.setattr(driver, "WRITE_CHUNK_UNITS", 7)
    bams, vcf_path, lib_json = three_sample_case(str(tmp_path))
    out_bam = str(tmp_path / "three_chunks.bam")
    run_w(bams, vcf_path, lib_json, out_bam)
    same_writes(out_bam, golden["three"])


def test_without_a_vcf_the_bam_holds_the_header_only(tmp_path, capsys):
    out_bam = str(tmp_path / "header.bam")
    classic.sv_genotype(T.IN_BAM, None, None, 20, 1, 1, 1000000, T.LIB_JSON, False, out_bam, None, False, None, 1e10,
                        engine=V.VerdictOracleEngine())
    assert "VCF not found" in capsys.readouterr().err
    f, records = all_records(out_bam)
    t = bam.AlignmentFile(T.IN_BAM, "rb")
    assert records == [] and f._header_bytes == t._header_bytes
    assert open(out_bam, "rb").read()[-28:] == bam.BGZF_EOF
    f.close()
    t.close()


def test_a_unit_skipped_by_max_reads_writes_none_of_its_reads(tmp_path):
    """--max_reads 300 skips one unit of the fixture (variant 99771).  Over a VCF of that line and its neighbours the dump equals,
    record for record, the dump of a run without the limit over the same VCF without the line -- and the line's own reads, which
    the run without the limit writes, are what is missing."""
    lines = open(T.IN_VCF).read().split("\n")
    head = [l for l in lines if l.startswith("#")]
    body = [l for l in lines if l and not l.startswith("#")]
    at = [i for i, l in enumerate(body) if l.split("\t")[2] == "99771"]
    assert len(at) == 1
    plain = lambda ls: [l for l in ls if "SVTYPE=BND" not in l]      # (a BND line without its mate would wait for it)
    near = plain(body[:at[0]])[-4:] + [body[at[0]]] + plain(body[at[0] + 1:])[:4]
    assert len(near) == 9 and "SVTYPE=BND" not in body[at[0]]
    paths = {}
    for name, chosen in (("with", near), ("without", [l for l in near if l.split("\t")[2] != "99771"])):
        paths[name] = str(tmp_path / (name + ".vcf"))
        with open(paths[name], "w") as f:
            f.write("\n".join(head + chosen) + "\n")
    limited = str(tmp_path / "limited.bam")
    vcf = run_w(T.IN_BAM, paths["with"], T.LIB_JSON, limited, max_reads=300)
    columns = {l.split("\t")[2]: l.split("\t")[9] for l in vcf if l and not l.startswith("#")}
    assert columns["99771"] == "./." and sum(c == "./." for c in columns.values()) == 1      # such a unit exists
    others = str(tmp_path / "others.bam")
    run_w(T.IN_BAM, paths["without"], T.LIB_JSON, others)
    assert V.written_records(limited) == V.written_records(others)
    unlimited = str(tmp_path / "unlimited.bam")
    run_w(T.IN_BAM, paths["with"], T.LIB_JSON, unlimited)
    assert len(V.written_records(unlimited)[0]) > len(V.written_records(others)[0])


# ------------------------------------------------------------------------------------------ what -w refuses
def _call(tmp_path, engine=None, **kw):
    out_bam = str(tmp_path / "refused.bam")
    with open(T.IN_VCF) as inf:
        classic.sv_genotype(T.IN_BAM, inf, io.StringIO(), 20, 1, 1, 1000000, T.LIB_JSON, False, out_bam, None, False, None, 1e10,
                            engine=engine or V.VerdictOracleEngine(), **kw)


@pytest.mark.parametrize("kw, text", [({"reader": "native"}, "keeps no reads"), ({"reader": "device"}, "keeps no reads"),
                                      ({"geometry": "device"}, "no canonical records")])
def test_routes_without_reads_or_records_are_refused(tmp_path, kw, text):
    with pytest.raises(ValueError, match=text):
        _call(tmp_path, **kw)
    assert not os.path.exists(str(tmp_path / "refused.bam"))


def test_an_engine_without_verdicts_is_refused(tmp_path):
    with pytest.raises(ValueError, match="supports_verdicts"):
        _call(tmp_path, engine=T.oracle_engine)
    assert not os.path.exists(str(tmp_path / "refused.bam"))


def test_the_sharded_driver_is_refused(tmp_path):
    with open(T.IN_VCF) as inf, pytest.raises(ValueError, match="every rank would write the same file"):
        sharded.sv_genotype_sharded(T.IN_BAM, inf, io.StringIO(), 20, 1, 1, 1000000, T.LIB_JSON, False, str(tmp_path / "refused.bam"),
                                    None, False, None, 1e10, rank=0, world=2, engine=V.VerdictOracleEngine())
    assert not os.path.exists(str(tmp_path / "refused.bam"))


def test_pack_fragments_side_table_leaves_the_records_alone():
    """pack_fragments(..., side_table=True): the same records, and per fragment its record span, the ungated is_ref_seq hits
    and the split objects behind the k-th seq / clip entries -- over the fake-read sites of tests/golden/fake_sites.json.gz"""
    import fakereads
    import goldenio
    from svtyper_amd import fragments as fr
    from svtyper_amd import packer

    class Lib:
        def __init__(self, L):
            self.name, self.mean, self.sd = L["name"], goldenio.fh(L["mean"]), goldenio.fh(L["sd"])
    g = goldenio.load("fake_sites.json.gz")
    n_spans = n_mapq0_hits = n_continued = 0
    for grp in g["groups"]:
        libs = [Lib(L) for L in grp["libraries"]]
        rg_to_lib = {rg: lib for lib, L in zip(libs, grp["libraries"]) for rg in L["readgroups"]}
        lib_index = {id(lib): i for i, lib in enumerate(libs)}
        for site in grp["sites"][:40]:
            fragments = {}
            for t in site["reads"]:
                r = fakereads.FakeRead(*t)
                if r.query_name in fragments:
                    fragments[r.query_name].add_read(r)
                else:
                    fragments[r.query_name] = fr.SamFragment(r, rg_to_lib[r.get_tag("RG")])
            plain = packer.pack_fragments(fragments, site["breakpoint"], lib_index, 20, 3)
            recs, spans = packer.pack_fragments(fragments, site["breakpoint"], lib_index, 20, 3, side_table=True)
            assert recs.tobytes() == plain.tobytes()
            assert [s.name for s in spans] == sorted(fragments)
            at = 0
            for s in spans:
                frag = fragments[s.name]
                assert s.first == at
                at += s.count
                assert len(s.ref_hits) == len(frag.primary_reads)
                assert sorted(map(id, s.seq + s.clip)) == sorted(map(id, frag.split_reads))
                assert all(not x.is_soft_clip for x in s.seq) and all(x.is_soft_clip for x in s.clip)
                assert s.count == max(1, (len(s.ref_hits) + 1) // 2, len(s.seq), len(s.clip))
                for k, (read, hit) in enumerate(zip(frag.primary_reads, s.ref_hits)):
                    gated = int(recs[s.first + k // 2]["rs_a" if k % 2 == 0 else "rs_b"])
                    assert gated == (min(read.mapping_quality, 255) if hit else 0)
                    n_mapq0_hits += bool(hit and read.mapping_quality == 0)
                n_spans += 1
                n_continued += s.count > 1
            assert at == len(recs)
    assert n_spans > 100 and n_mapq0_hits > 0 and n_continued > 0

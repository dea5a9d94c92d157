"""The tag grammar and the CIGAR operation classes of svtyper_amd/csrc/svt_record_rules.h (rr::walk_tags, op_ref / op_query /
op_aligned / op_clip) on the CPU, over the corpus of tests/grammarcases.py: every tag type, every B subtype with 0 / 1 / 3 / 17
elements, payloads that spell a tag inside another tag's value, RG and SA under a wrong type or twice, SA in front of RG, RG as
the last tag.  The host reader and the host form of the device walks share walk_tags, so neither can check the other's
grammar; here both are compared with sides that do not pass through it: grammarcases.spec_tags (the SAM specification's type
table, `struct` only) and the Python reader (svtyper_amd/bam.py), which are first compared with each other.
tests/test_record_grammar_device.py runs the same inputs through the three kernels.

Census of tests/data/NA12878.target_loci.sorted.bam (grammarcases.type_census over its 42 801 records): 171 204 tags of type
C and 173 169 of type Z -- and nothing else.  The fixture holds no A, c, s, S, i, I, f or H and no B array: for those, and for
anything in front of, between or behind RG and SA that is not a one-byte integer or a string, the corpus is the only test."""
import pytest

import grammarcases as G
import libscancases as lc
import test_native_reads as N
import walkcases as W
from svtyper_amd import bam, hip, native_reads as nr

MODES = [nr.COUNT_CLASSIC, nr.COUNT_SSO]
CENSUS = {"C": 171204, "Z": 173169}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("grammar")


@pytest.fixture(scope="module")
def evidence_unit(workdir):
    return G.evidence_input(workdir)


@pytest.fixture(scope="module")
def deep_unit(workdir):
    return G.deep_input(workdir)


@pytest.fixture(scope="module")
def library_bam(workdir):
    hip.build()
    b = nr.NativeBam(G.library_input(str(workdir / "grammar_lib.bam")))
    yield b
    b.close()


def test_census_of_the_fixture():
    assert G.type_census(W.FIXTURE_BAM) == CENSUS


def test_the_corpus_holds_what_it_is_there_for():
    seen, subtypes = set(), {}
    for rec in G.evidence_records():
        body = bw_record(rec)
        for _key, typ, at, size in G.walk_spec(body, G.tag_area(body)):
            seen.add(typ)
            if typ == "B":
                subtypes.setdefault(chr(body[at]), set()).add((size - 5) // G._SIZE[chr(body[at])])
    assert seen == set("AcCsSiIfZHB")
    assert set(subtypes) == set(G.SUBTYPES) and all(set(G.COUNTS) <= n for n in subtypes.values())
    last = bw_record(G.decorated([label for label, _ in G.CORPUS].index("arrays17_last"))[1])
    *_, (key, typ, at, size) = G.walk_spec(last, G.tag_area(last))
    assert typ == "B" and at + size == len(last)                      # an array ends the record
    assert len(G.evidence_records()) < 64


def bw_record(rec):
    import bamwriter as bw
    return bw.encode_record(rec)[0][4:]


@pytest.mark.parametrize("which", ["evidence", "deep", "library"])
def test_spec_tags_agrees_with_the_python_reader(which, evidence_unit, deep_unit, library_bam):
    """the reference first: the two independent statements of the grammar give the same first RG:Z and first SA:Z"""
    path = {"evidence": evidence_unit[1].bam.filename, "deep": deep_unit[1].bam.filename, "library": library_bam.filename}[which]
    n = n_sa = 0
    placed = [body for body in G.iter_records(path) if body[3] < 0x80]          # (fetch() leaves out the unplaced reads)
    reads = list(bam.AlignmentFile(path).fetch())
    assert len(reads) == len(placed)
    for body, read in zip(placed, reads):
        rg, sa = G.spec_tags(body)
        assert (read.get_tag("RG") if read.has_tag("RG") else None) == rg, read.query_name
        assert read.has_tag("SA") == (sa is not None), read.query_name
        if sa is not None:
            assert read.get_tag("SA") == sa, read.query_name
            n_sa += 1
        n += 1
    assert n == {"evidence": len(G.evidence_records()), "deep": G.N_DEEP, "library": G.N_LIBRARY}[which] and n_sa > 0


def _three(sites, sample, nbam, mode, max_reads=None):
    a = W.unit_arrays(sites, sample, nbam, mode)
    host = nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    walk = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    py = N._python_records(sites, sample, mode, max_reads)
    return host, walk, py


@pytest.mark.parametrize("mode", MODES)
def test_evidence_equals_the_python_reader(evidence_unit, mode):
    """svt_bam_evidence and the host walk against the Python reader + packer: offsets, records and skip flags, byte for byte;
    no unit falls back"""
    host, walk, py = _three(*evidence_unit, mode)
    assert not walk[3].any(), "flagged: %s" % [nr.WALK_REASONS[int(x)] for x in walk[3]]
    assert int(walk[4][0]) == len(G.evidence_records()) < 64
    assert N._same(host, py) and N._same(walk, py)
    assert len(py[1]) >= len(G.evidence_records()) and not py[2].any()
    sites, sample, nbam = evidence_unit                 # ... and the summaries, every field of every piece
    assert N._same(N._native_summaries(sites, sample, nbam, mode, None, 2), N._python_summaries(sites, sample, mode, None))


@pytest.mark.parametrize("mode", MODES)
def test_deep_unit_equals_the_python_reader(deep_unit, mode):
    host, walk, py = _three(*deep_unit, mode)
    assert not walk[3].any(), "flagged: %s" % [nr.WALK_REASONS[int(x)] for x in walk[3]]
    assert int(walk[4][0]) == G.N_DEEP > nr.walk_capacities()["reads_lds"]
    assert N._same(host, py) and N._same(walk, py) and len(py[1]) >= G.N_DEEP


def test_losing_or_inventing_a_tag_is_visible(tmp_path):
    """what makes a wrong skip wrong evidence and not just an error: the records of the split candidate differ between its SA,
    the SA that the payloads spell and no SA; the read group that the payloads spell is not the header's"""
    def records(name, tags):
        sites, sample, nbam = G.evidence_input(tmp_path, [W._read("s", 49_990, cigar="60M40S", tags=tags)], name)
        a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
        return nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)[1].tobytes()
    rg = ("RG", "Z", "rg")
    real, fake, none = (records("v%d" % k, [rg] + ([("SA", "Z", sa)] if sa else [])) for k, sa in enumerate((G.REAL_SA, G.FAKE_SA, None)))
    assert len({real, fake, none}) == 3
    with pytest.raises(hip.SvtyperHipError):
        records("other", [("RG", "Z", "other")])


def test_summaries_carry_the_sa_that_spec_tags_finds(evidence_unit):
    """per record: the read is of the one library (its RG is the header's, as spec_tags says) and the split piece of its
    summary is the first SA:Z entry of spec_tags -- or absent where spec_tags finds none"""
    sites, sample, nbam = evidence_unit
    recs = sorted(G.evidence_records(), key=lambda r: r["name"])
    off, frags, skipped = N._native_summaries(sites, sample, nbam, nr.COUNT_SSO, None, 1)
    py = N._python_summaries(sites, sample, nr.COUNT_SSO, None)
    assert N._same((off, frags, skipped), py) and len(frags) == len(recs)
    n_sa = 0
    for rec, f in zip(recs, frags):
        rg, sa = G.spec_tags(bw_record(rec))
        assert rg == "rg" and int(f["read"][0]["start"]) == rec["pos"], rec["name"]
        piece = f["seq"][1 if rec["cigar"] == "60M40S" or rec["cigar"] == "60M40H" else 0]
        if sa is None or rec["cigar"] == "100M":          # (an SA entry on an unclipped read leaves too little outside the overlap)
            assert not f["seq"]["flags"].any(), rec["name"]
            continue
        chrom, pos, strand, cigar, mapq, _nm = sa.rstrip(";").split(",")
        assert int(piece["flags"]) & 1 and (int(piece["tid"]), int(piece["start"]), int(piece["mapq"])) == (nbam.gettid(chrom), int(pos) - 1, int(mapq)), rec["name"]
        assert bool(int(piece["flags"]) & 2) == (strand == "-")
        n_sa += 1
    assert n_sa == len(G.CORPUS) + 1


# ---- the library walk ----------------------------------------------------------------------------------------------------------
def _spec_histograms(path, num_samp):
    """per library of lc.GROUPS the (template length, count) pairs in the order of their first record, from spec_tags' RG of
    every placed record with the QUALIFYING flags and tlen > 0; the first `num_samp` such records of a library when not 0"""
    import struct
    hists = [dict() for _ in lc.GROUPS]
    taken = [0] * len(lc.GROUPS)
    for body in G.iter_records(path):
        tid, flag, tlen = struct.unpack_from("<i", body, 0)[0], struct.unpack_from("<H", body, 14)[0], struct.unpack_from("<i", body, 28)[0]
        if tid < 0 or flag != lc.QUALIFYING or tlen <= 0:
            continue
        rg, _ = G.spec_tags(body)
        for k, group in enumerate(lc.GROUPS):
            if rg in group and (num_samp == 0 or taken[k] < num_samp):
                hists[k][tlen] = hists[k].get(tlen, 0) + 1
                taken[k] += 1
    return [list(h.items()) for h in hists]


@pytest.mark.parametrize("round_bytes", [0, lc.SMALL_ROUND])
@pytest.mark.parametrize("num_samp", [0, 150])
def test_library_walk(library_bam, num_samp, round_bytes):
    st = lc.compare(library_bam, lc.GROUPS, num_samp, round_bytes, route="walk_host", expect_reason=lc.WALK)
    assert st["host_reason"] is None and st["records_walked"] == G.N_LIBRARY
    assert (st["rounds"] > 1) == (round_bytes != 0)
    want = _spec_histograms(library_bam.filename, num_samp)
    assert all(sum(c for _, c in h) > 20 for h in want)
    walk = library_bam.scan_libraries(lc.GROUPS, num_samp, route="walk_host", round_bytes=round_bytes, ordered=True)
    assert [list(h) for _rl, h, _in, _tot in walk] == want
    assert [list(h) for _rl, h, _in, _tot in lc.host_scan(library_bam, lc.GROUPS, num_samp)] == want


# ---- outside the envelope ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["front", "behind"])
def test_an_array_of_an_unknown_subtype_is_malformed(tmp_path, where):
    """B:d is no array of the specification: the Python reader raises and the native walk stops there (it used to take four
    bytes per element and walk on).  In front of RG neither native side reaches the read group; behind RG the walk flags the
    unit as malformed and the host reader, which walks that far for a split candidate, fails the call."""
    rg, sa = ("RG", "Z", "rg"), ("SA", "Z", G.REAL_SA)
    tags = [G.UNKNOWN_SUBTYPE, rg, sa] if where == "front" else [rg, G.UNKNOWN_SUBTYPE, sa]
    host, walk, py, _ = N._corner(tmp_path, "subtype_" + where, [W._read("b", 49_990, cigar="60M40S", tags=tags)])
    assert py is None and N._reason(walk) == ("no_rg" if where == "front" else "malformed") and len(walk[1]) == 0
    assert isinstance(host, str) and ("RG tag" if where == "front" else "malformed") in host

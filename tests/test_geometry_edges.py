"""The boundary lattice of the geometry predicates (tests/geomcases.py, tests/golden/geometry_edges.json.gz: records, tallies
and results made by the REFERENCE) against every host evaluation of them: the Python reader (fragments.py + packer.py), the
native reader (svt_bam_evidence: svt_geometry_math.h in the reader's threads) and the host build of the evidence walk.  CPU only.

The reach test is a condition on the INPUTS: from the golden file and the census helper alone (a restatement of the reference's
predicates kept in tests/geomcases.py) every threshold has a fragment on both of its sides whose record, as the reference wrote
it, shows the verdict."""
import numpy as np
import pytest

import fakereads
import geomcases as G
import goldenio as gio
from svtyper_amd import evidence as ev
from svtyper_amd import fragments as fr
from svtyper_amd import native_reads as nr
from svtyper_amd import packer


@pytest.fixture(scope="module")
def golden():
    return gio.load("geometry_edges.json.gz")


@pytest.fixture(scope="module")
def reach(golden):
    """{(arrangement,) + event key + (verdict,): count} of the decisive events, every one checked against the reference's
    record; plus per-fragment facts for the count cases"""
    keys, frags = {}, []
    for grp in golden["groups"]:
        for site in grp["sites"]:
            cen = G.site_census(site, grp["libraries"])
            assert len(cen) == len(site["record_fragments"]), site["breakpoint"]["id"]
            arr, at = G.arrangement_of(site["breakpoint"]), 0
            for f, n in zip(cen, site["record_fragments"]):
                rows = site["records"][at:at + n]
                at += n
                frags.append((site["breakpoint"]["id"], f, rows))
                # every verdict of the restatement is the reference's, event or not
                if f["n_primary"] == 2:
                    for bit, name in ((1, "alt"), (2, "ref_a"), (4, "ref_b")):
                        assert bool(rows[0][G.ROW["flags"]] & bit) == f[name], (f["name"], name)
                for j, hit in enumerate(f["rs"]):
                    assert G.field_value(rows, ("rs", j)) == hit, (f["name"], "rs", j)
                for key, field, verdict, decisive in f["events"]:
                    if decisive:
                        assert G.field_value(rows, field) == verdict, (f["name"], key, field)
                        k = (arr,) + key + (verdict,)
                        keys[k] = keys.get(k, 0) + 1
            assert at == len(site["records"])
    return keys, frags


ARR = [(svtype, o1, o2, layout) for _, svtype, o1, o2, layout in G.ARRANGEMENTS]


def _straddle_keys(pred, side, rev, cis):
    """both sides of the near and of the far threshold of one side, the far one for every kind of flank"""
    out = []
    for ci in cis:
        ci = tuple(ci)
        if rev:    # inner < lo fails; inner > hi + flank fails
            out += [(pred, side, rev, "near", -1, ci, None, False), (pred, side, rev, "near", 0, ci, None, True)]
            out += [(pred, side, rev, "far", d, ci, fc, d <= 0) for d in (0, 1) for fc in ("int", "frac", "half")]
        else:      # inner > hi fails; inner < lo - flank fails
            out += [(pred, side, rev, "near", 0, ci, None, True), (pred, side, rev, "near", 1, ci, None, False)]
            out += [(pred, side, rev, "far", d, ci, fc, d >= 0) for d in (-1, 0) for fc in ("int", "frac", "half")]
    return out


def test_lattice_arrangements_are_what_the_corpus_says(golden):
    seen = {G.arrangement_of(s["breakpoint"]) for s in golden["groups"][0]["sites"]}
    assert set(ARR) <= seen and len(set(ARR)) == 12
    inter = [a for a in ARR if a[3] != "same"]
    assert {a[3] for a in inter} == {"inter", "inter_pos", "inter_tid"} and {(a[1], a[2]) for a in inter} == {
        (False, True), (True, False), (False, False), (True, True)}


def test_reach_pair_and_reference_straddles(reach):
    keys, _ = reach
    missing = []
    for arr in ARR:
        _, o1, o2, _ = arr
        want = _straddle_keys("alt", 1, o1, G.CIS) + _straddle_keys("alt", 2, o2, G.CIS)
        if arr[0] == "INV":
            want += _straddle_keys("alt_recip", 1, not o1, G.CIS) + _straddle_keys("alt_recip", 2, not o2, G.CIS)
        for pred in ("ref_a", "ref_b"):
            want += _straddle_keys(pred, 1, False, [(0, 0)]) + _straddle_keys(pred, 2, True, [(0, 0)])
        missing += [(arr,) + k for k in want if (arr,) + k not in keys]
    assert not missing, (len(missing), missing[:10])


def test_reach_is_ref_seq(reach):
    keys, _ = reach
    missing = []
    for arr in ARR:
        for side in ("A", "B"):
            for j in (0, 1):
                want = [("ref_seq", side, j, "start", d, 1, 1, "m", d <= 0) for d in (-1, 0, 1)]
                want += [("ref_seq", side, j, "end", d, 1, 1, "m", d >= 0) for d in (-1, 0, 1)]
                missing += [(arr,) + k for k in want if (arr,) + k not in keys]
    d = ("DEL", False, True, "same")
    want = []
    for d_ in (-1, 0, 1):
        want += [("ref_seq", "A", 0, "start", d_, 2, 2, "m", d_ <= 0), ("ref_seq", "A", 0, "end", d_, 1, 2, "m", d_ >= 0),     # xM yN zM, xM yD zM
                 ("ref_seq", "A", 0, "start", d_, 1, 1, "eqx", d_ <= 0), ("ref_seq", "A", 0, "end", d_, 1, 1, "eqx", d_ >= 0),  # = / X
                 ("ref_seq", "A", 0, "start", d_, 3, 4, "m", d_ <= 0), ("ref_seq", "A", 0, "end", d_, 3, 4, "m", d_ >= 0)]      # third of four
    want += [("ref_seq", "A", 0, "inside_ins", 0, 1, 1, "m", True), ("ref_seq", "A", 0, "inside", 0, 3, 4, "m", True),
             ("ref_seq", "B", 0, "inside", 0, 4, 4, "m", True), ("ref_seq", "A", 0, "inside", 0, 2, 4, "m", True),            # nearest two: 2nd and 4th
             ("ref_seq", "A", 2, "start", 0, 1, 1, "m", True)]                                                                 # a third primary
    # pos = m - 1, m, m + 1 at the start of a chromosome: (pos - m, start of the read)
    want += [("ref_seq_start_of_chrom", -1, 0, False), ("ref_seq_start_of_chrom", 0, 0, True), ("ref_seq_start_of_chrom", 0, 1, False),
             ("ref_seq_start_of_chrom", 1, 0, True), ("ref_seq_start_of_chrom", 1, 1, True), ("ref_seq_start_of_chrom", 1, 2, False)]
    missing += [(d,) + k for k in want if (d,) + k not in keys]
    assert not missing, (len(missing), missing[:10])


def test_reach_split_and_clip(reach):
    keys, _ = reach
    split = {}
    for k in keys:
        if k[1] == "split":
            arr, _, kind, piece, side, rev, d, verdict = k
            assert verdict == (abs(d) <= G.SLOP), k
            split.setdefault((arr, kind, piece, side, rev), set()).add(d)
    edge = {-4, -3, 3, 4}
    missing = []
    # SA candidates: the left piece against the left breakend, the right piece against the right one.  (Between chromosomes the
    # reference takes B for the left breakend and orders the pieces by the primary's clip: with strands (+, -) no piece of a
    # split read that follows the strands is compared with a breakend of its own chromosome, so that arrangement has none.)
    for arr in ARR:
        if arr == ("BND", False, True, "inter"):
            continue
        for piece in ("L", "R"):
            got = set().union(*[v for k, v in split.items() if k[:3] == (arr, "seq", piece)] or [set()])
            if not set(range(-5, 6)) <= got:
                missing.append((arr, "seq", piece, sorted(got)))
    # soft clips: DEL left / right, DUP swapped, INV either piece at either breakend
    for arr, plan in ((("DEL", False, True, "same"), [("L", "A"), ("R", "B")]), (("DUP", True, False, "same"), [("L", "B"), ("R", "A")]),
                      (("INV", False, False, "same"), [("L", "A"), ("L", "B"), ("R", "A"), ("R", "B")]),
                      (("INV", True, True, "same"), [("L", "A"), ("L", "B"), ("R", "A"), ("R", "B")])):
        for piece, side in plan:
            got = set().union(*[v for k, v in split.items() if k[:4] == (arr, "clip", piece, side)] or [set()])
            if not set(range(-5, 6)) <= got:
                missing.append((arr, "clip", piece, side, sorted(got)))
    # every (kind, piece, strand of the breakend) sees the whole of -5 .. +5 somewhere
    for kind in ("seq", "clip"):
        for piece in ("L", "R"):
            for rev in (False, True):
                got = set().union(*[v for k, v in split.items() if (k[1], k[2], k[4]) == (kind, piece, rev)] or [set()])
                if not set(range(-5, 6)) <= got:
                    missing.append((kind, piece, rev, sorted(got)))
    for arr in ARR:
        if not any(k[0] == arr and k[1] == "split_two_sa" for k in keys):
            missing.append((arr, "two SA entries"))
        if not any(k[0] == arr and k[1] == "split_wrong_chrom" for k in keys):
            missing.append((arr, "wrong chromosome"))
    assert edge <= set(range(-5, 6)) and not missing, missing[:10]


def test_reach_counts_ospan_and_empty_units(golden, reach):
    _, frags = reach
    by_primaries = {}
    for sid, f, rows in frags:
        by_primaries.setdefault(f["n_primary"], []).append((sid, f, rows))
    assert len(by_primaries[1]) > 100 and len(by_primaries[2]) > 1000
    three = by_primaries[3]
    assert three and all(len(rows) == 2 and rows[1][G.ROW["flags"]] & ev.REC_CONTINUATION for _, _, rows in three)
    assert any(rows[1][G.ROW["rs_a"]] > 0 for _, _, rows in three)                # the third primary's gated MAPQ, in the continuation
    two_clips = [rows for _, f, rows in frags if [k for k, _, _ in f["splits"]] == ["clip", "clip"]]
    assert two_clips and all(len(rows) == 2 and rows[0][G.ROW["clip_l"]] > 0 and rows[1][G.ROW["clip_r"]] > 0 for rows in two_clips)
    main, ospan = golden["groups"]
    twice = [s for s in main["sites"] if len({tuple(r) for r in s["reads"]}) < len(s["reads"])]
    assert [s["breakpoint"]["id"] for s in twice] == ["counts"]
    assert any(f["ref_a"] and f["ref_b"] for _, f, _ in frags)                    # a pair that straddles A and B at once
    # ospan at, one below and beyond the clamp
    assert [s["records"][0][0] for s in ospan["sites"]] == [2**31 - 2, 2**31 - 1, 2**31 - 1]
    assert [s["fits_int32"] for s in ospan["sites"]] == [True, True, False] and not ospan["bam"]
    assert [s["reads"][1][3] + 101 - s["reads"][0][3] for s in ospan["sites"]] == [2**31 - 2, 2**31 - 1, 2**31 + 5]
    # empty units: leading, two in a row in the middle, trailing
    empty = [k for k, s in enumerate(main["sites"]) if not s["reads"]]
    n = len(main["sites"])
    assert len(empty) == 4 and empty[0] == 0 and empty[3] == n - 1 and empty[2] == empty[1] + 1 and 1 < empty[1] < n - 3
    assert all(main["sites"][k]["records"] == [] and main["sites"][k]["result"]["formats"]["GT"] == "./." for k in empty)


def test_golden_is_the_corpus_of_the_generator(golden):
    """the committed reads are what tests/geomcases.py generates today (the golden is regenerated, not edited)"""
    groups = G.corpus()
    assert [g["name"] for g in groups] == [g["name"] for g in golden["groups"]]
    for made, kept in zip(groups, golden["groups"]):
        assert [s["breakpoint"] for s in made["sites"]] == [s["breakpoint"] for s in kept["sites"]]
        assert [[list(r.astuple()) for r in s["reads"]] for s in made["sites"]] == [s["reads"] for s in kept["sites"]]
    n_frag = sum(len(s["record_fragments"]) for g in golden["groups"] for s in g["sites"])
    assert 2000 < n_frag < 6000


# ------------------------------------------------------------------------------------------ (b) the Python reader
class _Lib:
    def __init__(self, name, mean, sd):
        self.name, self.mean, self.sd = name, mean, sd


def python_records(site, rg_to_lib, lib_index):
    frags = {}
    for t in site["reads"]:
        r = fakereads.FakeRead(*t)
        lib = rg_to_lib[r.get_tag("RG")]
        if r.query_name in frags:
            frags[r.query_name].add_read(r)
        else:
            frags[r.query_name] = fr.SamFragment(r, lib)
    return packer.pack_fragments(frags, site["breakpoint"], lib_index, 20, 3)


def assert_records_equal(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    for name in want.dtype.names:
        bad = np.nonzero(got[name] != want[name])[0]
        assert bad.size == 0, (where, name, bad[:5], got[name][bad[:5]], want[name][bad[:5]])


def test_python_reader_gives_the_reference_records_and_tallies(golden):
    from oracle import c_oracle
    from svtyper_amd.results import result_from_record
    for grp in golden["groups"]:
        libs = [_Lib(L["name"], gio.fh(L["mean"]), gio.fh(L["sd"])) for L in grp["libraries"]]
        rg_to_lib = {rg: lib for lib, L in zip(libs, grp["libraries"]) for rg in L["readgroups"]}
        lib_index = {id(lib): i for i, lib in enumerate(libs)}
        sites = []
        for site in grp["sites"]:
            got = python_records(site, rg_to_lib, lib_index)
            assert_records_equal(got, gio.records_from_rows(site["records"]), site["breakpoint"]["id"])
            sites.append(dict(site, records=[[int(x) for x in row] for row in got.tolist()]))
        # ... and from the Python reader's records the reference's tallies and results (CPU oracle engine)
        res = c_oracle.genotype_batch(gio.batch_from_sites(sites, grp["libraries"]), flags=ev.FLAG_SSO_ASSOCIATION)
        for k, s in enumerate(sites):
            for j, t in enumerate(gio.TALLIES):
                assert float(res.tallies[k, j]).hex() == s["tallies_sso"][t], (s["breakpoint"]["id"], t)
            gio.assert_result_equal(result_from_record(res.rec[k]), gio.golden_result(s["result"]), 0.0, s["breakpoint"]["id"])


# ------------------------------------------------------------------------------------------ (c), (d) the native builds
@pytest.fixture(scope="module")
def bam_groups(golden, tmp_path_factory):
    """[(group, sites, sample, nbam)] of the groups a BAM can carry (the 2^31 spans cannot: a BAM position is 32 bits and the
    index ends at 2^29)"""
    tmp = tmp_path_factory.mktemp("edges")
    out = []
    for grp in golden["groups"]:
        if grp["bam"]:
            out.append((grp,) + tuple(G.write_group_bam(tmp, grp, grp["libraries"])))
    assert len(out) == 1
    return out


def golden_unit_records(grp):
    want = [gio.records_from_rows(s["records"]) for s in grp["sites"]]
    return np.cumsum([0] + [len(w) for w in want]).astype(np.uint64), np.concatenate(want)


@pytest.mark.parametrize("mode,threads", [(nr.COUNT_SSO, 1), (nr.COUNT_CLASSIC, 3)])
def test_native_reader_gives_the_reference_records(bam_groups, mode, threads):
    import test_native_reads as N
    for grp, sites, sample, nbam in bam_groups:
        off, want = golden_unit_records(grp)
        got = N._native_records(sites, sample, nbam, mode, None if mode == nr.COUNT_CLASSIC else 1000, threads)
        assert not got[2].any() and np.array_equal(got[0], off)
        assert_records_equal(got[1], want, "svt_bam_evidence")
        py = N._python_records(sites, sample, mode, None if mode == nr.COUNT_CLASSIC else 1000)     # (the BAM carries the reads as meant)
        assert np.array_equal(py[0], off)
        assert_records_equal(py[1], want, "python reader on the BAM")


def test_host_walk_gives_the_reference_records(bam_groups):
    import walkcases as W
    for grp, sites, sample, nbam in bam_groups:
        off, want = golden_unit_records(grp)
        a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
        walk = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
        assert not np.asarray(walk[3]).any(), "a unit left the walk's envelope"
        assert not walk[2].any() and np.array_equal(walk[0], off)
        assert_records_equal(walk[1], want, "svt_bam_evidence_walk_host")


def test_the_five_positions_give_five_records():
    """the unit look-up test of tests/test_geometry_edges_device.py tells neighbouring units apart by these records"""
    spec = G.library_specs()[0]
    lib = _Lib(spec[0], spec[2], spec[3])
    recs = set()
    for pos in G.LOOKUP_POS_A:
        bp = {"id": "u", "svtype": "DEL", "var_length": 4000, "A": {"chrom": "1", "pos": pos, "ci": [0, 0], "is_reverse": False},
              "B": {"chrom": "1", "pos": 5000, "ci": [0, 0], "is_reverse": True}}
        f = fr.SamFragment(fakereads.FakeRead("f", 97, "1", 1000, "101M", 60, rg="rg0"), lib)
        f.add_read(fakereads.FakeRead("f", 145, "1", 1300, "101M", 37, rg="rg0"))
        recs.add(packer.pack_fragments({"f": f}, bp, {id(lib): 0}, 20, 3).tobytes())
    assert len(recs) == len(G.LOOKUP_POS_A)

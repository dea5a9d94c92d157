"""The concordance decision at the edges of its construction, on the CPU.  tests/golden/concordance_edges.json.gz holds what the
REFERENCE's SamFragment.p_concordant answers on the lattice of tests/concordcases.py (ratio 19 : 1 bins on both sides of the
boundary, thresholds capped at the largest count, one- and two-bin libraries, equal counts, zero bins, counts of 2^31 - 1,
negative keys and keys at +-2^29, the float key of a non-DEL unit integral and nearly so, libraries at the limits of the 16-bit
tables); this file requires, point by point and with no tolerance (booleans and integers only):

  * the golden is the lattice's, and holds both answers at h2 == 19 * h1;
  * oracle.py_oracle.p_concordant and the C oracle's svt_oracle_p_concordant give the golden's answers;
  * build_tables (svtyper_amd/csrc/svt_host_tables.h, driven by tests/native/host_tables_main.cpp, built with g++) makes the
    dense ranks of this suite's own threshold search, its `hist_rank[o - v] <= thr_rank[o]` is the golden's answer, narrow_bins
    flips between 32 767 and 32 768 distinct values and fast_geometry is as its comments say;
  * the packed encoder accepts the probe batches of the families it can express.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import concordcases as CC
import goldenio as gio
from oracle import c_oracle, py_oracle
from svtyper_amd.evidence import LibraryTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


@pytest.fixture(scope="module")
def golden():
    return gio.load("concordance_edges.json.gz")


def golden_cases(golden):
    """[(Lib of concordcases, LibraryTable from the GOLDEN's histogram, points, answers as bools)], small families then wide"""
    out = []
    for L, g in zip(CC.small_libraries(), golden["libraries"]):
        table = LibraryTable.from_counter({int(k): int(c) for k, c in g["hist"].items()}, gio.fh(g["mean"]), gio.fh(g["sd"]), g["name"])
        out.append((L, table, [(o, v) for o, v in g["points"]], [c == "1" for c in g["answers"]]))
    for recipe, g in zip(CC.WIDE_RECIPES, golden["wide"]):
        L = CC.wide_library(recipe)
        out.append((L, L.table(), L.points, [c == "1" for c in g["answers"]]))
    return out


def test_the_golden_is_the_lattice(golden):
    libs = CC.small_libraries()
    assert [g["name"] for g in golden["libraries"]] == [L.name for L in libs] and len(libs) >= 27
    for L, g in zip(libs, golden["libraries"]):
        assert g["family"] == L.family and {int(k): c for k, c in g["hist"].items()} == L.hist, L.name
        assert gio.fh(g["mean"]) == L.mean and gio.fh(g["sd"]) == L.sd
        assert [tuple(p) for p in g["points"]] == L.points and len(g["answers"]) == len(L.points) and set(g["answers"]) <= {"0", "1"}
        assert 2 * L.sd < 10 or L.family == "nondel"
        v = L.mean + L.sd * 3
        assert (v == np.floor(v)) == (L.name == "nondel_integral")
    assert [g["recipe"] for g in golden["wide"]] == list(CC.WIDE_RECIPES)
    for g in golden["wide"]:
        L = CC.wide_library(g["recipe"])
        assert g["sha256"] == CC.wide_sha256(g["recipe"]) and g["n_bins"] == len(L.counts) and g["key_min"] == CC.WIDE_KEY_MIN
        assert g["n_points"] == len(L.points) == len(g["answers"]) and 1900 <= len(L.points) <= 2100
        assert gio.fh(g["mean"]) == L.mean and gio.fh(g["sd"]) == L.sd
    assert set(CC.SMALL_FAMILIES) == {L.family for L in libs}
    assert os.path.getsize(os.path.join(gio.GOLDEN, "concordance_edges.json.gz")) < 200_000


def test_the_golden_stands_on_both_sides(golden):
    """at h2 == 19 * h1, where p is 0.5 and only the rounding decides, the reference answers True at least three times and False
    at least three times; both answers in every family; the families hold what their names say"""
    at_boundary = {True: 0, False: 0}
    by_family = {}
    for L, table, points, answers in golden_cases(golden):
        by_family.setdefault(L.family, set()).update(answers)
        if L.family != "ratio":
            continue
        hist = L.hist
        for (o, v), a in zip(points, answers):
            h1, h2 = hist.get(o, 0), hist.get(o - v, 0)
            if h1 > 0 and h2 == 19 * h1:
                at_boundary[a] += 1
                assert (L.name.endswith("_true")) == a or h1 != hist[201], (L.name, o, v)
    assert at_boundary[True] >= 3 and at_boundary[False] >= 3, at_boundary
    assert all(s == {True, False} for s in by_family.values()), by_family
    assert len(CC.family("ratio")) >= 8 and all(10 <= len(L.hist) <= 14 for L in CC.family("ratio"))
    for L in CC.family("ratio"):
        h1 = L.hist[201]
        assert {19 * h1 + d for d in range(-2, 3)} | {0, 1, h1} <= set(L.hist.values())
    cap = CC.family("capped")[0]
    hmax = max(cap.hist.values())
    assert any(cap.hist.get(o, 0) > hmax / 19 and cap.hist.get(o - v, 0) == hmax for o, v in cap.points)
    assert len(set(CC.family("flat")[0].hist.values())) == 1 and len(CC.family("flat")[0].hist) == 50
    sp = CC.family("sparse")[0]
    zero = lambda k: sp.hist.get(k, 0) == 0
    assert any(min(sp.hist) < o < max(sp.hist) and zero(o) and not zero(o - v) for o, v in sp.points)
    assert any(not zero(o) and zero(o - v) and min(sp.hist) < o - v < max(sp.hist) for o, v in sp.points)
    assert any(zero(o) and zero(o - v) for o, v in sp.points)
    hg = CC.family("huge")[0]
    assert max(hg.hist.values()) == 2 ** 31 - 1 and sum(hg.hist.values()) > 2 ** 32
    assert {(2 ** 31 - 1) // 19 + d for d in range(-2, 3)} <= set(hg.hist.values())
    assert [min(L.hist) for L in CC.family("negative")] == [-40, -2 ** 29 - 1, -2 ** 29, 2 ** 29, 2 ** 29 + 1]
    assert max(CC.family("negative")[0].hist) == 40
    assert all(max(o for o, _v in L.points) == 2 ** 31 - 1 for L in CC.family("nondel")[1:])


def test_both_oracles_answer_as_the_reference(golden):
    n = 0
    for L, table, points, answers in golden_cases(golden):
        lib = py_oracle._Lib(table)
        for (o, v), want in zip(points, answers):
            assert py_oracle.p_concordant(lib, o, v) is want, ("py_oracle", L.name, o, v)
            assert c_oracle.p_concordant(table, o, v) is want, ("c_oracle", L.name, o, v)
        n += len(points)
    assert n > 16000


# ------------------------------------------------------------------------------------------ build_tables
@pytest.fixture(scope="module")
def host_tables(tmp_path_factory):
    """run(tables) -> [(rc, narrow_bins, fast_geometry, thr_rank, hist_rank)] from build_tables, one call per library"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("host_tables")
    exe = str(tmp / "host_tables")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native", "host_tables_main.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd[:5] + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + cmd[5:], capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()):      # (a g++ without the sanitizer runtimes)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(tables):
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<I", len(tables)))
            for t in tables:
                h = np.ascontiguousarray(t.hist, dtype="<u4")
                f.write(struct.pack("<iIdd", int(t.key_min), len(h), float(t.mean), float(t.sd)) + h.tobytes())
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        blob, at, out = open(dst, "rb").read(), 0, []
        for _t in tables:
            rc, narrow, fast, n = struct.unpack_from("<iIII", blob, at)
            bins = np.frombuffer(blob, dtype=[("thr", "<i4"), ("hist", "<u4")], count=n, offset=at + 16)
            at += 16 + 8 * n
            out.append((rc, bool(narrow), bool(fast), bins["thr"].astype(np.int64), bins["hist"].astype(np.int64)))
        assert at == len(blob) and len(r.stdout.splitlines()) == len(tables)
        return out
    return run


@pytest.fixture(scope="module")
def built(golden, host_tables):
    cases = golden_cases(golden)
    return cases, host_tables([table for _L, table, _p, _a in cases])


def bin_index(table, key):
    """the bin of an integral Counter key; beyond the histogram the sentinel"""
    i = key - int(table.key_min)
    return i if 0 <= i < len(table.hist) else len(table.hist)


def second_key(table, o, v):
    """o - v as the Counter sees it (parsers.py:874-878): without a var_length the float o - (mean + 3 sd), which names a bin only
    when it is integral; None = no bin"""
    if v is not None:
        return o - v
    key = o - (table.mean + table.sd * 3)
    return int(key) if key == np.floor(key) else None


def decide(table, thr_rank, hist_rank, o, v):
    k2 = second_key(table, o, v)
    i2 = len(table.hist) if k2 is None else bin_index(table, k2)
    return bool(hist_rank[i2] <= thr_rank[bin_index(table, o)])


def test_build_tables_makes_the_dense_ranks_of_the_threshold_search(built):
    """Bin{thr, hist} of every library equals this suite's own restatement (concordcases.dense_ranks): the thresholds found on
    the expression, the ranks counted from 0 among the distinct values of hist + thr + {0}, the sentinel {-1, rank of 0} last"""
    cases, tabs = built
    for (L, table, _p, _a), (rc, _narrow, _fast, thr_rank, hist_rank) in zip(cases, tabs):
        assert rc == 0 and len(thr_rank) == len(table.hist) + 1, L.name
        want_thr, want_hist, _n = CC.dense_ranks(table.hist)
        assert thr_rank[-1] == -1 and hist_rank[-1] == 0, L.name
        assert np.array_equal(hist_rank, want_hist), (L.name, np.nonzero(hist_rank != want_hist)[0][:5])
        assert np.array_equal(thr_rank, want_thr), (L.name, np.nonzero(thr_rank != want_thr)[0][:5])


def test_the_rank_compare_is_the_reference_at_every_point(built):
    cases, tabs = built
    n = 0
    for (L, table, points, answers), (_rc, _narrow, _fast, thr_rank, hist_rank) in zip(cases, tabs):
        for (o, v), want in zip(points, answers):
            assert decide(table, thr_rank, hist_rank, o, v) is want, (L.name, o, v)
        n += len(points)
    assert n > 16000


def test_the_rank_compare_is_the_oracle_over_all_bin_pairs(built):
    """the small families: every pair of keys from one below to one above the histogram, negative spans included (the golden
    has the non-negative ones; a Counter does not care), against py_oracle -- which the golden has just been compared with"""
    cases, tabs = built
    for (L, table, _p, _a), (_rc, _narrow, _fast, thr_rank, hist_rank) in zip(cases, tabs):
        if L.family == "wide":
            continue
        lib = py_oracle._Lib(table)
        keys = range(int(table.key_min) - 1, int(table.key_min) + len(table.hist) + 1)
        for a in keys:
            for b in keys:
                assert decide(table, thr_rank, hist_rank, a, a - b) is py_oracle.p_concordant(lib, a, a - b), (L.name, a, b)
        if L.family == "nondel":
            for o in keys:
                assert decide(table, thr_rank, hist_rank, o, None) is py_oracle.p_concordant(lib, o, None), (L.name, o)


def test_narrow_bins_flips_between_the_two_libraries_built_for_it(built):
    """16-bit ranks hold 32 767 distinct values and not one more; the limits are the ones the code states"""
    cases, tabs = built
    narrow = {L.name: t[1] for (L, _t, _p, _a), t in zip(cases, tabs)}
    values = {L.name: CC.dense_ranks(table.hist)[2] for L, table, _p, _a in cases if L.family == "wide"}
    assert values["wide_values_32767"] == 32767 and values["wide_values_32768"] == 32768
    assert narrow["wide_values_32767"] is True and narrow["wide_values_32768"] is False
    assert all(ok for name, ok in narrow.items() if name != "wide_values_32768")
    assert len(CC.wide_counts("wide_bins_lds_fit")) == CC.LDS_MAX_BINS == 15167 and len(CC.wide_counts("wide_bins_lds_over")) == 15168
    text = lambda name: open(os.path.join(CSRC, name)).read()
    assert "if (vals.size() > %d) T.narrow_bins = false;" % CC.NARROW_VALUES in text("svt_host_tables.h")
    assert "single_lds + kWavesPerBlock * kStreamRingBytes <= 96 * 1024" in text("svt_batch_create.h")
    assert "const size_t single_lds = kSBins + T.bins.size() * kLdsBin;" in text("svt_batch_create.h")
    assert "constexpr uint32_t kSBins = kSWhi + 2 * 32 * 4;" in text("svt_wg_parts.h") and CC.K_SBINS == 4864


def test_fast_geometry_is_as_the_comments_say(built):
    """|key_min| <= 2^29, and a mean + 3 sd further than 4e-6 from an integer"""
    cases, tabs = built
    fast = {L.name: t[2] for (L, _t, _p, _a), t in zip(cases, tabs)}
    want_slow = {"keymin_m%d" % (2 ** 29 + 1), "keymin_p%d" % (2 ** 29 + 1), "nondel_integral", "nondel_3e-6"}
    assert want_slow <= set(fast) and {"keymin_m%d" % 2 ** 29, "keymin_p%d" % 2 ** 29, "nondel_5e-6", "negative_m40"} <= set(fast)
    assert {name for name, ok in fast.items() if not ok} == want_slow


# ------------------------------------------------------------------------------------------ the packed encoder
PACKED_FAMILIES = ("ratio", "capped", "tiny", "flat", "sparse", "huge")


def packed_libraries():
    """what the packed format is asked to take: the probe batches of these families and of the key_min = -40 library, restricted
    to var_length >= 0 (the format declines a negative DEL length, svt_pack.cpp)"""
    return [L for L in CC.small_libraries() if L.family in PACKED_FAMILIES or L.name == "negative_m40"]


def test_the_packed_encoder_accepts_the_probe_batches():
    from svtyper_amd import hip
    libs = packed_libraries()
    assert len(libs) == 8 + 1 + 7 + 1 + 1 + 1 + 1
    for L in libs:
        batch, where = CC.probe_batch([L], only_nonnegative=True)
        assert len(where) > len(L.points) // 3
        packed = hip.PackedEvidence.try_pack(batch)
        assert packed is not None, "%s (family %s): declined" % (L.name, L.family)
        with packed:
            assert packed.n_units == batch.n_units
    batch, _ = CC.probe_batch(libs, only_nonnegative=True)
    with hip.PackedEvidence.try_pack(batch) as packed:
        assert packed.n_units == batch.n_units
    # ... and what it declines, for the reason it documents
    L = CC.family("ratio")[0]
    batch, _ = CC.probe_batch([L])
    assert (batch.units["var_length"] < 0).any()
    with pytest.raises(hip.SvtyperHipError, match="negative DEL length"):
        hip.PackedEvidence(batch)
    for name in ("keymin_p%d" % (2 ** 29 + 1), "nondel_integral"):
        L = [x for x in CC.small_libraries() if x.name == name][0]
        batch, _ = CC.probe_batch([L], only_nonnegative=True)
        with pytest.raises(hip.SvtyperHipError, match="library geometry outside the packed format's range"):
            hip.PackedEvidence(batch)

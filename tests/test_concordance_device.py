"""GPU: every consumer of the concordance tables (svt_host_tables.h: rank(hist[o - v]) <= rank(thr[o])) against
tests/golden/concordance_edges.json.gz, the lattice on which the REFERENCE's SamFragment.p_concordant decided
(tests/concordcases.py; the host side of it is tests/test_concordance_host.py).  No tolerance anywhere: tallies are compared as
bit patterns, verdicts as bytes.

Two batch shapes per set of libraries:

  probe   one unit per point with exactly one record (concordcases.probe_batch).  The expected tallies follow from the golden
          boolean alone -- ref_span = pm60 * pm60 / 2 or 0.0, for DEL alt_span = 0.0 or pm60 * pm60 --; no oracle takes part.
          The zeroing rules (classic.py:425-435) cannot fire on such a unit: alt_seq + alt_clip is 0 and alt_span stays below
          1, so the test reads got.tallies of every unit as they are.
  mixed   units of 1, 63, 64, 65, 129 and 300 records drawn from the points that share a var_length, varied MAPQs, every
          straddle-bit combination, continuation records: the C oracle's results through assert_parity (the oracle itself
          equals the golden point by point, test_concordance_host.py), and DeviceBatch.verdicts() against verdictcases.restate.

through the resident and the one-shot entry with ALL_FLAGS, the table modes 0, 1 and 2 (table_mode() asserted each time), the
streaming, split (K = 2, 4) and cooperative kernels by the debug hooks, the verdict kernel, and packed evidence of one library,
of up to 256 and of more than 256 libraries.
"""
import ctypes as C

import numpy as np
import pytest

import concordcases as CC
import goldenio as gio
import verdictcases as V
from svtyper_amd import evidence as ev
from test_hip_parity import ALL_FLAGS, assert_parity

pytestmark = pytest.mark.gpu

ONE_LIBRARY, WINDOWS, GENERAL = CC.ONE_LIBRARY, CC.WINDOWS, CC.GENERAL
DEFAULT_COOP = 1 << 40
# (name, svt_debug_small_kind, svt_debug_coop max units): the rule (cooperative for launches this small), the cooperative kernel
# off (the rule then takes lanes per unit), the streaming kernel, two and four lanes per unit
KINDS = (("coop", 0, DEFAULT_COOP), ("coop off", 0, 0), ("stream", 1, DEFAULT_COOP), ("split 2", 3, DEFAULT_COOP), ("split 4", 4, DEFAULT_COOP))


@pytest.fixture(scope="module")
def answers():
    """{library name: [bool per point]} from the golden"""
    g = gio.load("concordance_edges.json.gz")
    out = {L["name"]: [c == "1" for c in L["answers"]] for L in g["libraries"]}
    out.update({W["recipe"]: [c == "1" for c in W["answers"]] for W in g["wide"]})
    for L in CC.small_libraries():
        assert len(out[L.name]) == len(L.points)
    return out


def _hooks():
    from svtyper_amd import hip
    lib = hip.load()
    lib.svt_debug_coop.argtypes = [C.c_uint64, C.c_uint32]
    lib.svt_debug_coop.restype = None
    lib.svt_debug_small_kind.argtypes = [C.c_int]
    return lib


def fast_geometry(table):
    """build_tables' rule, whose outcome on these libraries test_concordance_host.py asserts"""
    v = table.mean + table.sd * 3
    return abs(table.key_min) <= 2 ** 29 and abs(v - round(v)) > 4e-6


def natural_mode(batch):
    """the mode svt_batch_create.h must give these batches: every library here fits 16-bit ranks and LDS unless it is one of
    the wide ones, so only the geometry and the number of libraries decide"""
    if not all(fast_geometry(t) for t in batch.libs):
        return GENERAL
    if len(batch.libs) > 1:
        return WINDOWS
    return ONE_LIBRARY if len(batch.libs[0].hist) <= CC.LDS_MAX_BINS else GENERAL


def through_every_pass(batch, device, check, mode=None, kinds=KINDS, flags_list=ALL_FLAGS):
    """check(results, flags, label) on the result records of `batch` from the resident and the one-shot entry, in the batch's
    own table mode under every kernel kind, and in the general mode"""
    from svtyper_amd import hip
    lib = _hooks()
    mode = natural_mode(batch) if mode is None else mode
    try:
        for general in (0, ev.FLAG_GENERAL_TABLES):
            want_mode = GENERAL if general else mode
            for name, kind, coop in (kinds if want_mode != GENERAL else kinds[:1]):
                lib.svt_debug_small_kind(kind)
                lib.svt_debug_coop(coop, 0)
                for flags in flags_list:
                    label = (name, flags | general)
                    with hip.DeviceBatch(batch, device, flags | general) as d:
                        assert d.table_mode() == want_mode, (label, d.table_mode())
                        d.genotype(sync=True)
                        check(d.results(), flags, ("resident",) + label)
                    check(hip.genotype_batch(batch, device, flags | general), flags, ("one-shot",) + label)
    finally:
        lib.svt_debug_small_kind(0)
        lib.svt_debug_coop(DEFAULT_COOP, 0)


def probe_check(batch, where, libs, answers):
    want = CC.probe_tallies(batch, [answers[libs[k].name][j] for k, j in where])
    want_bits = want.view(np.uint64)

    def check(res, flags, label):
        got = np.ascontiguousarray(res.tallies).view(np.uint64)
        bad = np.nonzero((got != want_bits).any(axis=1))[0]
        assert bad.size == 0, "%r: %d of %d units; first: library %s point %r: tallies %r, the reference's answer gives %r" % (
            label, bad.size, batch.n_units, libs[where[bad[0]][0]].name, libs[where[bad[0]][0]].points[where[bad[0]][1]],
            res.tallies[bad[0]].tolist(), want[bad[0]].tolist())
    return check


def mixed_check(batch):
    from oracle import c_oracle
    want = {sso: c_oracle.genotype_batch(batch, flags=sso) for sso in (0, ev.FLAG_SSO_ASSOCIATION)}
    assert set(np.diff(batch.rec_offset.astype(np.int64)).tolist()) == set(CC.MIXED_SIZES)

    def check(res, flags, label):
        try:
            assert_parity(res, want[flags & ev.FLAG_SSO_ASSOCIATION])
        except AssertionError as e:
            raise AssertionError("%r: %s" % (label, e))
    return check


def verdicts_check(batch, device, mode=None):
    from svtyper_amd import hip
    want = V.restate(batch)
    mode = natural_mode(batch) if mode is None else mode
    for flags, want_mode in ((0, mode), (ev.FLAG_GENERAL_TABLES, GENERAL)):
        with hip.DeviceBatch(batch, device, flags) as d:
            got = d.verdicts()
            assert d.table_mode() == want_mode
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "flags %#x, record %d of %d: kernel %#x, restatement %#x, record %r" % (
            flags, bad[0], got.size, got[bad[0]], want[bad[0]], batch.records[bad[0]])
    return want


def run_set(libs, device, answers, hints=1):
    batch, where = CC.probe_batch(libs, hints=hints)
    through_every_pass(batch, device, probe_check(batch, where, libs, answers))
    mixed = CC.mixed_batch(libs, hints=hints)
    through_every_pass(mixed, device, mixed_check(mixed))
    return verdicts_check(mixed, device)


# ------------------------------------------------------------------------------------------ canonical records
@pytest.mark.parametrize("family", CC.SMALL_FAMILIES)
def test_each_library_alone(hip_device, answers, family):
    """one library per batch: tables in LDS (mode 0) under every kernel kind, through L2 (mode 2) where the geometry asks for it
    and wherever FLAG_GENERAL_TABLES does"""
    modes = set()
    for L in CC.family(family):
        run_set([L], hip_device, answers)
        modes.add(natural_mode(CC.probe_batch([L])[0]))
    assert modes == ({ONE_LIBRARY, GENERAL} if family in ("negative", "nondel") else {ONE_LIBRARY})


def test_the_verdicts_reach_both_tags_through_the_lattice(hip_device):
    """from the restatement of the mixed ratio batch: "alt branch taken" tagged A and R and "ref branch taken" tagged A and R on
    DEL pairs with two non-zero MAPQs, i.e. through p_concordant alone"""
    mixed = CC.mixed_batch(CC.family("ratio"), hints=0)
    want = verdicts_check(mixed, hip_device)
    both = (mixed.records["mapq_a"] > 0) & (mixed.records["mapq_b"] > 0)
    for taken, tag in ((V.ALT_TAKEN, V.ALT_A), (V.REF_TAKEN, V.REF_A)):
        sel = both & ((want & taken) != 0)
        assert ((want[sel] & tag) != 0).any() and ((want[sel] & tag) == 0).any()


@pytest.mark.parametrize("hints", [1, 4, 0], ids=["own library", "windows of 4", "no hints"])
def test_all_ratio_libraries_together(hip_device, answers, hints):
    """library windows (mode 1): of one library each (the one-library consumer, record_single), of four, and without hints the
    whole batch as one window of eight (record_window)"""
    libs = CC.family("ratio")
    assert natural_mode(CC.probe_batch(libs, hints=hints)[0]) == WINDOWS
    run_set(libs, hip_device, answers, hints)


@pytest.mark.parametrize("hints", [1, 5, 0], ids=["own library", "windows of 5", "no hints"])
def test_ratio_tiny_and_sparse_as_one_batch(hip_device, answers, hints):
    libs = CC.family("ratio") + CC.family("tiny") + CC.family("sparse")
    assert len(libs) == 16 and natural_mode(CC.probe_batch(libs, hints=hints)[0]) == WINDOWS
    run_set(libs, hip_device, answers, hints)


# ------------------------------------------------------------------------------------------ the wide family
@pytest.mark.parametrize("recipe", CC.WIDE_RECIPES)
def test_wide_libraries(hip_device, answers, recipe):
    """libraries at the limits of the 16-bit tables: 15 167 bins still take the one-library LDS mode, 15 168 the general one
    (svt_batch_create.h: single_lds); 32 767 / 32 768 distinct values (narrow_bins) lie beyond that limit on either side, so
    both run in the general mode -- the flip of narrow_bins itself is asserted on the host"""
    L = CC.wide_library(recipe)
    want_mode = ONE_LIBRARY if recipe == "wide_bins_lds_fit" else GENERAL
    batch, where = CC.probe_batch([L])
    assert natural_mode(batch) == want_mode and 1900 <= batch.n_units <= 2100
    through_every_pass(batch, hip_device, probe_check(batch, where, [L], answers), mode=want_mode)
    mixed = CC.mixed_batch([L])
    through_every_pass(mixed, hip_device, mixed_check(mixed), mode=want_mode, flags_list=ALL_FLAGS[:2])
    verdicts_check(mixed, hip_device, want_mode)


# ------------------------------------------------------------------------------------------ packed evidence
def packed_libraries():
    from test_concordance_host import packed_libraries as host_list
    return host_list()


def through_packed(batch, device, check, many=False):
    from svtyper_amd import hip
    packed = hip.PackedEvidence.try_pack(batch, many_libraries=many)
    assert packed is not None, "the packed format declined %d libraries" % len(batch.libs)
    with packed:
        for flags in ALL_FLAGS:
            check(hip.genotype_packed(packed, device, flags), flags, ("packed one-shot", flags))
            with hip.DeviceBatch.from_packed(packed, device, flags) as d:
                assert d.layout_name() == "packed"
                d.genotype(sync=True)
                check(d.results(), flags, ("packed resident", flags))


def test_packed_evidence_of_one_library(hip_device, answers):
    for L in packed_libraries():
        batch, where = CC.probe_batch([L], only_nonnegative=True)
        through_packed(batch, hip_device, probe_check(batch, where, [L], answers))
        mixed = CC.mixed_batch([L], only_nonnegative=True)
        through_packed(mixed, hip_device, mixed_check(mixed))


@pytest.mark.parametrize("n_libs,many", [(0, False), (256, False), (300, True), (65536, True)],
                         ids=["the 19 libraries", "256 libraries", "300 libraries", "65 536 libraries"])
def test_packed_evidence_of_several_libraries(hip_device, answers, n_libs, many):
    """2 to 256 libraries, and more than 256 with many_libraries=True: two-bin fillers between the lattice's libraries, which
    sit at the lowest and the highest indices"""
    libs = packed_libraries()
    tables, index = (None, None) if not n_libs else CC.with_fillers(libs, n_libs)
    if n_libs:
        assert index[0] == 0 and index[-1] == n_libs - 1 and len(tables) == n_libs
    batch, where = CC.probe_batch(libs, index=index, tables=tables, only_nonnegative=True)
    assert int((batch.records["flags"] >> ev.REC_LIB_SHIFT).max()) == (n_libs or len(libs)) - 1
    through_packed(batch, hip_device, probe_check(batch, where, libs, answers), many)
    if n_libs <= 300:
        mixed = CC.mixed_batch(libs, index=index, tables=tables, only_nonnegative=True)
        through_packed(mixed, hip_device, mixed_check(mixed), many)

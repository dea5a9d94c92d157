"""GPU: the bytes of svt_verdict_kernel (svt_batch_verdicts, DeviceBatch.verdicts()) against the Python restatement of the six
bits (tests/verdictcases.py: restate, after svtyper/classic.py:317-408 with oracle.py_oracle.p_concordant) -- byte for byte, so no
tolerance: every bit is a comparison the reference makes, and the device's integer test for p_concordant (svt_host_tables.h) is
held to the reference point by point on the lattice of tests/concordcases.py (test_concordance_host.py, test_concordance_device.py:
the same bytes there on histograms in exact ratio 19 : 1, at the caps and at the limits of the tables).  Over the 211 fixture units, the boundary lattice of the geometry predicates and a synthetic batch of 300
libraries with DEL units on both sides of 2 sd, non-DEL units whose float Counter key is and is not integral, spans in the
sentinel bin, units of 0, 1, 63, 64, 65 and 129 records (a wavefront strides over a unit's records by 64), an empty first and
last unit and a skipped one."""
import numpy as np
import pytest

import goldenio as gio
import verdictcases as V
from svtyper_amd import evidence as ev

pytestmark = pytest.mark.gpu

ONE_LIBRARY, WINDOWS, GENERAL = 0, 1, 2      # DeviceBatch.table_mode()


def device_verdicts(batch, device, flags=0):
    from svtyper_amd import hip
    with hip.DeviceBatch(batch, device, flags) as d:
        return d.verdicts(), d.table_mode()


def same(got, want, batch):
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "record %d of %d: kernel %#x, restatement %#x, record %r" % (
        bad[0], got.size, got[bad[0]], want[bad[0]], batch.records[bad[0]])


@pytest.fixture(scope="module")
def synthetic():
    """(batch, restatement): 300 libraries, every third with an integral mean + 3 sd -- which keeps the batch out of the LDS modes"""
    batch = V.synthetic_batch()
    return batch, V.restate(batch)


@pytest.fixture(scope="module")
def windowed():
    """(batch, restatement): 40 libraries, one window per unit, no integral mean + 3 sd: the pass takes library windows"""
    batch = V.synthetic_batch(n_libs=40, seed=6, integral_every=0)
    return batch, V.restate(batch)


@pytest.mark.parametrize("flags", [0, ev.FLAG_SSO_ASSOCIATION], ids=["classic", "sso"])
def test_fixture_units(hip_device, flags):
    g = gio.load("fixture_sites.json.gz")
    assert len(g["sites"]) == 211
    batch = gio.batch_from_sites(g["sites"], g["libraries"])
    want = V.restate(batch)
    got, mode = device_verdicts(batch, hip_device, flags)
    assert mode == ONE_LIBRARY
    same(got, want, batch)
    assert all(((want & bit) != 0).any() and ((want & bit) == 0).any() for bit in (1, 2, 4, 8, 16, 32))


def test_geometry_lattice(hip_device):
    g = gio.load("geometry_edges.json.gz")
    n = 0
    for grp in g["groups"]:
        batch = gio.batch_from_sites(grp["sites"], grp["libraries"])
        got, _ = device_verdicts(batch, hip_device)
        same(got, V.restate(batch), batch)
        n += batch.n_records
    assert n > 500


def test_the_restatement_reaches_every_bit_both_ways(synthetic):
    """from the restatement alone: each bit set and clear somewhere; "alt branch taken, tag R" both through p_concordant (a DEL
    pair with two non-zero MAPQs) and through a zero MAPQ; both sides of the gate; the sentinel bin; every unit size"""
    batch, want = synthetic
    for bit in (1, 2, 4, 8, 16, 32):
        assert ((want & bit) != 0).any() and ((want & bit) == 0).any(), bit
    assert not (want & 0xC0).any()
    rec = batch.records
    unit_of = np.repeat(np.arange(batch.n_units), np.diff(batch.rec_offset.astype(np.int64)))
    is_del = batch.units["svtype"][unit_of] == 0
    taken_r = (want & 3) == 1
    both_mapq = (rec["mapq_a"] > 0) & (rec["mapq_b"] > 0)
    assert (taken_r & is_del & both_mapq).any()                    # p_conc made it R
    assert (taken_r & ~both_mapq).any()                            # a zero MAPQ made it R
    assert (taken_r & ~is_del).any() and not (taken_r & ~is_del & both_mapq).any()
    assert ((want & 3) == 3)[is_del].any() and ((want & 3) == 3)[~is_del].any()
    # the small-deletion gate: straddle bits on the record, no branch taken
    sd2 = np.array([2 * t.sd for t in batch.libs])[(rec["flags"] >> ev.REC_LIB_SHIFT) & 0xFFFF]
    gated = is_del & (batch.units["pos_delta"][unit_of] < sd2)
    straddles = ((rec["flags"] & 7) != 0) & ((rec["flags"] & ev.REC_HAS_PAIR) != 0)
    assert (gated & straddles).any() and not (want[gated] & 15).any()
    assert (is_del & ~gated & ((want & 5) != 0)).any()
    # continuation records carry bits 4 and 5 only, the records of the skipped unit nothing
    cont = (rec["flags"] & ev.REC_CONTINUATION) != 0
    assert cont.any() and not (want[cont] & 15).any() and (want[cont] & 48).any()
    skipped = (batch.units["flags"][unit_of] & ev.UNIT_SKIP) != 0
    assert skipped.any() and not want[skipped].any()
    # spans beyond a library's histogram (the sentinel bin), on pairs whose ref-straddle branch is taken
    key_max = np.array([t.key_min + len(t.hist) - 1 for t in batch.libs])[(rec["flags"] >> ev.REC_LIB_SHIFT) & 0xFFFF]
    assert ((rec["ospan_len"] > key_max) & ((want & 4) != 0)).any()
    sizes = set(np.diff(batch.rec_offset.astype(np.int64)).tolist())
    assert {0, 1, 63, 64, 65, 129} <= sizes
    assert batch.rec_offset[1] == 0 and batch.rec_offset[-1] == batch.rec_offset[-2]       # empty first and last unit
    assert len(batch.libs) == 300 and (rec["flags"] >> ev.REC_LIB_SHIFT).max() == 299
    # non-DEL units whose float key o - (mean + 3 sd) is integral, and ones where it is not
    v = np.array([t.mean + t.sd * 3 for t in batch.libs])
    assert (v == np.floor(v)).any() and (v != np.floor(v)).any()


def test_synthetic_batch_of_300_libraries(hip_device, synthetic):
    batch, want = synthetic
    got, mode = device_verdicts(batch, hip_device)
    assert mode == GENERAL
    same(got, want, batch)


def test_the_highest_library_index(hip_device, fixture_library):
    """65 536 libraries, the units name 0..2 and 65 533..65 535: every library is read through its own descriptor"""
    import manylibcases
    batch = manylibcases.highest_library(fixture_library)
    assert int((batch.records["flags"] >> ev.REC_LIB_SHIFT).max()) == 65535
    want = V.restate(batch)
    assert (want[((batch.records["flags"] >> ev.REC_LIB_SHIFT) & 0xFFFF) >= 65533] & 15).any()
    got, _ = device_verdicts(batch, hip_device)
    same(got, want, batch)


def test_the_same_bytes_whatever_mode_the_pass_runs_in(hip_device, windowed):
    from svtyper_amd import hip
    from svtyper_amd.evidence import SegmentedBatch
    batch, want = windowed
    got, mode = device_verdicts(batch, hip_device)
    assert mode == WINDOWS
    same(got, want, batch)
    got, mode = device_verdicts(batch, hip_device, ev.FLAG_GENERAL_TABLES)
    assert mode == GENERAL
    same(got, want, batch)
    # the records handed over in three pieces, cut inside units: the joined array counts
    cuts = [0, batch.n_records // 3 + 1, 2 * batch.n_records // 3 + 5, batch.n_records]
    pieces = SegmentedBatch(batch.rec_offset, batch.units, [batch.records[a:b] for a, b in zip(cuts, cuts[1:])], batch.libs)
    with hip.DeviceBatch.from_segments(pieces, hip_device) as d:
        same(d.verdicts(), want, batch)
    # one library: tables in LDS for the pass, the same bytes as under the general mode
    one = V.synthetic_batch(n_libs=1, seed=7, integral_every=0, sizes=(129, 64, 65))
    want_one = V.restate(one)
    got, mode = device_verdicts(one, hip_device)
    assert mode == ONE_LIBRARY
    same(got, want_one, one)
    got, mode = device_verdicts(one, hip_device, ev.FLAG_GENERAL_TABLES)
    assert mode == GENERAL
    same(got, want_one, one)


def test_results_are_the_same_bytes_with_the_call_before_after_and_absent(hip_device, windowed):
    from svtyper_amd import hip
    batch, want = windowed
    with hip.DeviceBatch(batch, hip_device) as d:
        d.genotype()
        absent = d.results().rec.tobytes()
    with hip.DeviceBatch(batch, hip_device) as d:
        before = d.verdicts()
        d.genotype()
        res_before = d.results().rec.tobytes()
        after = d.verdicts()
        res_after = d.results().rec.tobytes()
    assert res_before == absent and res_after == absent
    same(before, want, batch)
    same(after, want, batch)


def test_engine_puts_the_verdicts_beside_the_records(hip_device, windowed):
    from svtyper_amd.pipeline import HipEngine
    batch, want = windowed
    plain = HipEngine(hip_device)
    assert plain.supports_verdicts and plain(batch).verdicts is None
    res = HipEngine(hip_device, verdicts=True)(batch)
    same(res.verdicts, want, batch)
    assert res.rec.tobytes() == plain(batch).rec.tobytes()
    same(plain(batch, verdicts=True).verdicts, want, batch)


def test_a_packed_batch_and_a_wrong_count_are_refused(hip_device):
    import ctypes as C
    from svtyper_amd import hip
    one = V.synthetic_batch(n_libs=1, seed=7, integral_every=0, sizes=(5, 64))
    packed = hip.PackedEvidence.try_pack(one)
    assert packed is not None
    with packed, hip.DeviceBatch.from_packed(packed, hip_device) as d:
        assert d.layout_name() == "packed"
        with pytest.raises(hip.SvtyperHipError, match="error -1: .*packed evidence has no canonical records"):
            d.verdicts()
    with hip.DeviceBatch(one, hip_device) as d:
        out = np.zeros(one.n_records + 1, np.uint8)
        for n in (one.n_records - 1, one.n_records + 1):
            rc = d._lib.svt_batch_verdicts(d._h, C.c_void_p(out.ctypes.data), n)
            assert rc == -1 and b"rec_offset[n_units]" in d._lib.svt_last_error()
        assert not out.any()

"""The device reader (svt_bam_evidence_device: svt_evidence_kernel.h + the host fallback) against the shipped host reader
(svt_bam_evidence): the resident batch's records and offsets read back from HBM are the host reader's byte for byte, the
fallback count is the number of units the same walk flags on the CPU, units outside the envelope come back with the host's
records or the host's error, and the genotype pass on the produced batch gives the bits it gives on svt_batch_create's."""
import numpy as np
import pytest

import walkcases as W
from svtyper_amd import evidence as ev, hip, native_reads as nr

pytestmark = pytest.mark.gpu

MODES = [(nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 120), (nr.COUNT_CLASSIC, 150)]


def _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION, ev.FLAG_SSO_ASSOCIATION | ev.FLAG_RESULT96, 0)):
    a = W.unit_arrays(sites, sample, nbam, mode)
    want = nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    cpu = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    head = W.header_batch(sample, a[1])
    stats = None
    for fl in flags:
        d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, head, 0, fl, 2)
        off, recs = nr.batch_records(d)
        print("units %d records %d skipped %d host units %d (%s) reads walked %d" % (
            len(sites), len(recs), int(skipped.sum()), stats["units_host"], stats["units_host_by_reason"], stats["reads_walked"]))
        assert np.array_equal(skipped, want[2]), "skip flags differ"
        assert np.array_equal(off, want[0]), "record counts differ"
        assert recs.tobytes() == want[1].tobytes(), "records differ"
        assert stats["units_host"] == int(np.count_nonzero(cpu[3]))
        units = head.units.copy()
        units["flags"] = np.where(want[2] != 0, ev.UNIT_SKIP, 0)
        ref = hip.DeviceBatch(ev.EvidenceBatch(want[0], units, want[1], head.libs, 1.0, 1.0), 0, fl)
        d.genotype()
        ref.genotype()
        assert d.results().rec.tobytes() == ref.results().rec.tobytes(), "genotype results differ (flags %#x)" % fl
        d.close()
        ref.close()
    return stats, want


@pytest.mark.parametrize("mode,max_reads", MODES)
def test_fixture_records_in_hbm_equal_the_host_reader(mode, max_reads):
    sites, sample, nbam = W.fixture_input()
    stats, want = _compare(sites, sample, nbam, mode, max_reads)
    assert stats["units_host"] == 0
    assert len(want[1]) > 5000 or want[2].any()


@pytest.mark.parametrize("seed", W.SYNTHETIC_SEEDS)
@pytest.mark.parametrize("sa_first", [False, True])
def test_synthetic_bams_equal_the_host_reader(tmp_path, seed, sa_first):
    sites, sample, nbam = W.synthetic_input(tmp_path, seed, sa_first=sa_first, tied_names=(seed % 2 == 0))
    for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_CLASSIC, 90), (nr.COUNT_SSO, 200)):
        stats, _ = _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION,))
        assert stats["units_host"] == 0


@pytest.mark.parametrize("case", ["reads", "name", "cigar", "sa_entries", "no_rg", "unknown_rg", "malformed_sa"])
def test_units_outside_the_envelope_are_the_host_readers(tmp_path, case):
    records, reason, host_fails = W.envelope_cases(nr.walk_capacities())[case]
    sample, nbam = W.open_sample(W.write_case(tmp_path, case, records), W.INFO)
    sites = [{"breakpoint": W.SITE}]
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1])
    if host_fails:
        with pytest.raises(hip.SvtyperHipError) as host_err:
            nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
        with pytest.raises(hip.SvtyperHipError) as dev_err:
            nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1)
        assert str(dev_err.value) == str(host_err.value)
        return
    stats, want = _compare(sites, sample, nbam, nr.COUNT_SSO, None)
    assert stats["units_host"] == 1 and stats["units_host_by_reason"] == {reason: 1}
    assert len(want[1]) > 0


def test_first_failing_unit_in_unit_order_gives_the_error():
    """Two units that both go to the host reader and fail there with different texts, on two threads: the call fails with the
    text of the one that comes first in unit order, whichever thread finishes first.  Both are preset by the arena's planner
    (a window on a reference the header does not have: "BAM read error"; an svtype behind BND: "bad svtype"), so no walk runs
    over them."""
    sites, sample, nbam = W.fixture_input()
    a = W.unit_arrays(sites[:3], sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1])
    texts = ("BAM read error", "bad svtype")
    for bad_tid, bad_svtype, first in ((1, 2, 0), (2, 1, 1)):
        win, bps = a[0].copy(), a[1].copy()
        win["tid_a"][bad_tid] = len(nbam.references) + 1
        bps["svtype"][bad_svtype] = 200
        with pytest.raises(hip.SvtyperHipError) as err:
            nbam.evidence_device(win, bps, a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 2)
        assert texts[first] in str(err.value) and texts[1 - first] not in str(err.value)


def test_fake_read_bams_equal_the_host_reader(tmp_path):
    for sites, sample, nbam in W.fake_inputs(tmp_path):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 30), (nr.COUNT_CLASSIC, 25)):
            stats, _ = _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION, 0))
            assert stats["units_host"] == 0


def test_three_bam_golden_inputs_equal_the_host_reader(tmp_path):
    for sites, sample, nbam in W.three_bam_inputs(tmp_path):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000)):
            stats, _ = _compare(sites, sample, nbam, mode, max_reads, flags=(0, ev.FLAG_RESULT96))
            assert stats["units_host"] == 0


@pytest.mark.parametrize("mode", [nr.COUNT_CLASSIC, nr.COUNT_SSO])
def test_max_reads_boundaries(tmp_path, mode):
    sites, sample, nbam = W.boundary_input(tmp_path, 37)
    for limit in (35, 36, 37, 38):
        stats, want = _compare(sites, sample, nbam, mode, limit, flags=(0,))
        assert stats["units_host"] == 0
        assert bool(want[2][0]) == (limit < (37 if mode == nr.COUNT_SSO else 36))


def test_truncated_last_record_is_the_host_readers(tmp_path):
    """(passes on the CPU first: tests/test_evidence_walk_host.py)  The host reader either gives records or fails: the device
    route does the same, through the fallback."""
    sites, sample, nbam = W.truncated_input(tmp_path)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1])
    try:
        want = nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    except hip.SvtyperHipError as host_err:
        with pytest.raises(hip.SvtyperHipError) as dev_err:
            nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1)
        assert str(dev_err.value) == str(host_err)
        return
    d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1)
    off, recs = nr.batch_records(d)
    assert stats["units_host_by_reason"] == {"range": 1}
    assert np.array_equal(off, want[0]) and recs.tobytes() == want[1].tobytes()


def test_no_units():
    sites, sample, nbam = W.fixture_input()
    a = W.unit_arrays(sites[:1], sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1][:0])
    d, skipped, stats = nbam.evidence_device(a[0][:0], a[1][:0], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1)
    off, recs = nr.batch_records(d)
    assert len(skipped) == 0 and off.tolist() == [0] and len(recs) == 0 and stats["n_units"] == 0

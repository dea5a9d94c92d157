"""The deep tier of the device reader (svt_evidence_deep_kernel: one workgroup per unit of 1 025 .. 16 384 kept reads, its tables
in a slice of an HBM workspace) against the shipped host reader svt_bam_evidence, through svt_bam_evidence_device and
svt_bam_evidence_device_inflate: the records read back from HBM, their offsets and the skip flags are the host reader's byte for
byte, no unit of up to 16 384 reads goes to the host for `reads`, and svt_evidence_deep_stats counts what the deep kernel took.
(The same inputs pass on the CPU first: tests/test_deep_units_host.py.)"""
import numpy as np
import pytest

import deepcases as D
import walkcases as W
from svtyper_amd import classic, native_reads as nr, singlesample

pytestmark = pytest.mark.gpu
INFLATE = ["host", "device"]
MAX_WORKSPACE = 256 << 20


def _device(sites, sample, nbam, mode, max_reads, inflate):
    """(host reader's result, kept reads per unit by the CPU walk, stats of the device call); asserts the bytes"""
    a, want = D.host_reader(sites, sample, nbam, mode, max_reads)
    cpu = D.walk(nbam, a, mode, max_reads, "evidence_walk_open_host" if inflate == "device" else "evidence_walk_host")
    head = W.header_batch(sample, a[1])
    d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, head, 0, 0, 2, inflate=inflate)
    try:
        off, recs = nr.batch_records(d)
    finally:
        d.close()
    print("inflate %s mode %d max_reads %s: units %d records %d host units %d (%s) deep %s" % (
        inflate, mode, max_reads, len(sites), len(recs), stats["units_host"], stats["units_host_by_reason"], stats["deep"]))
    assert np.array_equal(skipped, want[2]), "skip flags differ"
    assert np.array_equal(off, want[0]), "record counts differ"
    assert recs.tobytes() == want[1].tobytes(), "records differ"
    assert stats["deep"] == nr.deep_stats()
    assert stats["deep"]["workspace_bytes"] <= MAX_WORKSPACE
    return want, cpu, stats


def _assert_deep_stats(stats, kept):
    """`kept`: kept reads per unit of the units the deep kernel is expected to take"""
    assert stats["deep"]["units_deep"] == len(kept) and stats["deep"]["reads_deep"] == int(sum(kept))
    assert (stats["deep"]["workspace_bytes"] > 0) == (len(kept) > 0)
    assert stats["deep"]["workspace_bytes"] % 1179648 == 0 and stats["deep"]["workspace_bytes"] // 1179648 <= max(len(kept), 0)


@pytest.mark.parametrize("inflate", INFLATE)
@pytest.mark.parametrize("n_reads", D.BOUNDARIES + (D.OVER,))
def test_tier_boundaries(tmp_path, hip_device, n_reads, inflate):
    sites, sample, nbam = W.boundary_input(tmp_path, n_reads)
    want, cpu, stats = _device(sites, sample, nbam, nr.COUNT_SSO, None, inflate)
    assert int(cpu[4][0]) == n_reads and len(want[1]) == n_reads
    if n_reads > D.DEEP:
        assert stats["units_host"] == 1 and stats["units_host_by_reason"] == {"reads": 1}
        _assert_deep_stats(stats, [])
    else:
        assert stats["units_host"] == 0 and stats["units_host_by_reason"].get("reads", 0) == 0
        _assert_deep_stats(stats, [n_reads] if n_reads > D.LDS else [])


@pytest.mark.parametrize("inflate", INFLATE)
@pytest.mark.parametrize("name", sorted(D.REALISTIC))
def test_realistic_deep_units(tmp_path, hip_device, name, inflate):
    sites, sample, nbam, (lo, hi) = D.realistic_input(tmp_path, name)
    for mode, max_reads in D.MODES:
        want, cpu, stats = _device(sites, sample, nbam, mode, max_reads, inflate)
        assert stats["units_host"] == 0 and stats["units_host_by_reason"].get("reads", 0) == 0
        if max_reads == 1000:
            assert want[2][0] == 1
            _assert_deep_stats(stats, [])               # (the count pass meets the limit: the unit is skipped, not deep)
        else:
            assert lo <= int(cpu[4][0]) <= hi and want[2][0] == 0 and len(want[1]) > 0
            _assert_deep_stats(stats, [int(cpu[4][0])])


@pytest.mark.parametrize("inflate", INFLATE)
@pytest.mark.parametrize("case", ["prefixes", "behind_the_key", "one_name", "name_cap"])
def test_adversarial_names(tmp_path, hip_device, case, inflate):
    sites, sample, nbam = D.adversarial_input(tmp_path, case)
    records = D.adversarial_cases()[case]
    for mode in (nr.COUNT_CLASSIC, nr.COUNT_SSO):
        want, cpu, stats = _device(sites, sample, nbam, mode, None, inflate)
        assert stats["units_host"] == 0 and len(want[1]) > 0
        if case in D.EQUAL_KEY_NAMES:                     # whole-name compares between equal keys: the unit keeps every record
            assert D.names_behind_equal_keys(records) == D.EQUAL_KEY_NAMES[case] and int(cpu[4][0]) == len(records)
        _assert_deep_stats(stats, [int(cpu[4][0])])


@pytest.mark.parametrize("inflate", INFLATE)
def test_mixed_call_sends_only_the_over_deep_units_to_the_host(tmp_path, hip_device, inflate):
    sites, sample, nbam = D.mixed_input(tmp_path)
    want, cpu, stats = _device(sites, sample, nbam, nr.COUNT_CLASSIC, None, inflate)
    shallow, deep, over = D.tiers(cpu[4])
    assert len(over) == 2 and len(deep) >= 2 and any(cpu[4][u] > 0 for u in shallow)
    assert stats["units_host"] == len(over) and stats["units_host_by_reason"] == {"reads": len(over)}
    _assert_deep_stats(stats, [int(cpu[4][u]) for u in deep])


@pytest.mark.parametrize("inflate", INFLATE)
def test_more_deep_units_than_workspace_slices(tmp_path, hip_device, inflate):
    """240 deep units of 1 100 reads: the workspace has 227 slices (256 MiB / 1 179 648 bytes), so the first workgroups take a
    second unit each"""
    sites, sample, nbam = D.many_deep_input(tmp_path, 240)
    want, cpu, stats = _device(sites, sample, nbam, nr.COUNT_SSO, None, inflate)
    assert (cpu[4] == 1100).all() and stats["units_host"] == 0
    assert stats["deep"]["units_deep"] == 240 and stats["deep"]["reads_deep"] == 240 * 1100
    assert stats["deep"]["workspace_bytes"] == 227 * 1179648 <= MAX_WORKSPACE


@pytest.mark.parametrize("inflate", INFLATE)
@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_drivers_over_a_deep_bam_give_the_native_readers_vcf(tmp_path, hip_device, driver, inflate):
    bam, vcf, lib_json = D.driver_case(tmp_path)

    def run(name, **kw):
        path = str(tmp_path / (name + ".vcf"))
        with open(vcf) as f, open(path, "w") as out:
            if driver == "classic":
                classic.sv_genotype(bam, f, out, 20, 1, 1, 1000000, lib_json, False, None, None, False, None, 1e10, **kw)
            else:
                singlesample.sso_genotype(bam, f, out, 20, 1, 1, 1000000, lib_json, False, None, False, 100000, 1e10, None, 1000, **kw)
        return [l for l in open(path).read().split("\n") if not l.startswith("##fileDate=")]

    stats = {}
    device = run("device", reader="device", inflate=inflate, stats=stats)
    native = run("native", reader="native")
    assert device == native and sum(1 for l in native if l and not l.startswith("#")) == 5
    d = stats["device_reader"]
    print(d)
    assert d["units_host"] == 0 and d["deep"]["units_deep"] == d["n_units"] >= 4 and d["deep"]["reads_deep"] > d["n_units"] * D.LDS   # every unit is a deep one
    assert 0 < d["deep"]["workspace_bytes"] <= MAX_WORKSPACE

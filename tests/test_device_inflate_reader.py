"""The device reader with the BGZF inflate on the GPU (svt_bam_evidence_device_inflate): tests/test_device_reader.py's comparison
restated for the new entry -- records and offsets read back from HBM, skip flags and genotype results are the host reader's --
and, through the public interface, both drivers and both command lines with reader="device", inflate="device"."""
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_host_pipeline as H
import test_multisample_qual as M
import test_walk_open_host as O
import walkcases as W
from svtyper_amd import classic, evidence as ev, hip, native_reads as nr, sharded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(H.HERE)
MODES = [(nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 120), (nr.COUNT_CLASSIC, 150)]


def _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION, ev.FLAG_SSO_ASSOCIATION | ev.FLAG_RESULT96, 0)):
    a = W.unit_arrays(sites, sample, nbam, mode)
    want = nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    cpu = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    head = W.header_batch(sample, a[1])
    stats = None
    for fl in flags:
        d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, head, 0, fl, 2, inflate="device",
                                                 count_host_blocks=True)
        off, recs = nr.batch_records(d)
        print("units %d records %d skipped %d host units %d (%s) inflate %s" % (
            len(sites), len(recs), int(skipped.sum()), stats["units_host"], stats["units_host_by_reason"], stats["inflate"]))
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
    assert stats["units_host"] == 0 and stats["inflate"]["blocks_failed"] == 0
    assert stats["inflate"]["blocks_inflated"] >= stats["inflate"]["blocks_host_route"] > 0
    assert len(want[1]) > 5000 or want[2].any()


@pytest.mark.parametrize("seed", W.SYNTHETIC_SEEDS)
def test_synthetic_bams_equal_the_host_reader(tmp_path, seed):
    sites, sample, nbam = W.synthetic_input(tmp_path, seed, tied_names=(seed % 2 == 0))
    for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_CLASSIC, 90), (nr.COUNT_SSO, 200)):
        stats, _ = _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION,))
        assert stats["units_host"] == 0


def test_fake_read_and_three_bam_inputs_equal_the_host_reader(tmp_path):
    for sites, sample, nbam in list(W.fake_inputs(tmp_path)) + list(W.three_bam_inputs(tmp_path)):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 30), (nr.COUNT_CLASSIC, 25)):
            stats, _ = _compare(sites, sample, nbam, mode, max_reads, flags=(ev.FLAG_SSO_ASSOCIATION, 0))
            assert stats["units_host"] == 0


@pytest.mark.parametrize("mode", [nr.COUNT_CLASSIC, nr.COUNT_SSO])
def test_max_reads_boundaries(tmp_path, mode):
    sites, sample, nbam = W.boundary_input(tmp_path, 37)
    for limit in (35, 36, 37, 38):
        stats, want = _compare(sites, sample, nbam, mode, limit, flags=(0,))
        assert stats["units_host"] == 0
        assert bool(want[2][0]) == (limit < (37 if mode == nr.COUNT_SSO else 36))


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
            nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1, inflate="device")
        assert str(dev_err.value) == str(host_err.value)
        return
    stats, want = _compare(sites, sample, nbam, nr.COUNT_SSO, None)
    assert stats["units_host"] == 1 and stats["units_host_by_reason"] == {reason: 1}
    assert len(want[1]) > 0


def test_truncated_last_record_is_the_host_readers(tmp_path):
    sites, sample, nbam = W.truncated_input(tmp_path)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1])
    try:
        want = nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    except hip.SvtyperHipError as host_err:
        with pytest.raises(hip.SvtyperHipError) as dev_err:
            nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1, inflate="device")
        assert str(dev_err.value) == str(host_err)
        return
    d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1, inflate="device")
    off, recs = nr.batch_records(d)
    assert stats["units_host_by_reason"] == {"range": 1}
    assert np.array_equal(off, want[0]) and recs.tobytes() == want[1].tobytes()


def test_a_corrupted_member_sends_exactly_the_units_over_it_to_the_host(tmp_path):
    sites, _sample, _nbam = W.fixture_input()
    path, _at = O.corrupted_fixture(tmp_path)
    info = json.load(open(os.path.join(W.DATA, "NA12878.bam.json")))
    sample, nbam = W.open_sample(path, info)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    cpu = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    over = np.flatnonzero(cpu[3] != 0)
    clear = np.flatnonzero(cpu[3] == 0)
    assert over.size and clear.size
    head = W.header_batch(sample, a[1][clear])
    want = nbam.evidence(a[0][clear], a[1][clear], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    d, skipped, stats = nbam.evidence_device(a[0][clear], a[1][clear], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 2, inflate="device")
    off, recs = nr.batch_records(d)
    assert stats["units_host"] == 0 and np.array_equal(off, want[0]) and recs.tobytes() == want[1].tobytes()
    # all units: exactly those over the member go to the host reader -- which gives their records, or its error text
    head = W.header_batch(sample, a[1])
    try:
        want = nbam.evidence(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    except hip.SvtyperHipError as host_err:
        with pytest.raises(hip.SvtyperHipError) as dev_err:
            nbam.evidence_device(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 2, inflate="device")
        assert str(dev_err.value).split(":")[-1] == str(host_err).split(":")[-1]
        return
    d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 2, inflate="device")
    off, recs = nr.batch_records(d)
    assert stats["units_host"] == over.size and stats["units_host_by_reason"] == {"range": int(over.size)}
    assert stats["inflate"]["blocks_failed"] == 1
    assert np.array_equal(off, want[0]) and recs.tobytes() == want[1].tobytes()


def test_no_units():
    sites, sample, nbam = W.fixture_input()
    a = W.unit_arrays(sites[:1], sample, nbam, nr.COUNT_SSO)
    head = W.header_batch(sample, a[1][:0])
    d, skipped, stats = nbam.evidence_device(a[0][:0], a[1][:0], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, 0, 0, 1, inflate="device")
    off, recs = nr.batch_records(d)
    assert len(skipped) == 0 and off.tolist() == [0] and len(recs) == 0 and stats["n_units"] == 0
    assert stats["inflate"]["blocks_inflated"] == 0


# ---- the public interface ----------------------------------------------------------------------------------------------------------
KW = dict(reader="device", inflate="device")


@pytest.mark.parametrize("cores", [None, 2])
def test_sso_genotype_reproduces_the_expected_vcf(tmp_path, hip_device, cores):
    out = str(tmp_path / "out.vcf")
    stats = {}
    H.run_sso(out, None, cores, stats=stats, **KW)
    H.same_vcf(out, H.EXPECTED)
    d = stats["device_reader"]
    print(d)
    assert d["n_units"] == 211 and d["units_host"] == 0 and d["n_records"] > 5000
    assert d["inflate"]["blocks_inflated"] > 0 and d["inflate"]["blocks_failed"] == 0 and d["inflate"]["compressed_bytes"] > 0


def test_sv_genotype_reproduces_the_expected_vcf(tmp_path, hip_device):
    out = str(tmp_path / "out.vcf")
    stats = {}
    H.run_classic(out, None, stats=stats, **KW)
    H.same_vcf(out, H.EXPECTED)
    assert stats["device_reader"]["n_units"] == 211 and stats["device_reader"]["units_host"] == 0
    assert stats["device_reader"]["inflate"]["blocks_inflated"] > 0


def test_two_bams_sum_quals_golden(tmp_path, hip_device):
    out = str(tmp_path / "out.vcf")
    with open(H.IN_VCF) as inf, open(out, "w") as outf:
        classic.sv_genotype(H.IN_BAM + "," + H.IN_BAM, inf, outf, 20, 1, 1, 1000000, H.LIB_JSON, False, None, None, True,
                            None, 1e10, **KW)
    want = gzip.open(os.path.join(H.HERE, "golden", "example.twice.sumquals.gt.vcf.gz"), "rt").read().split("\n")
    M._same([l for l in open(out).read().split("\n") if not l.startswith("##fileDate=")], want)


@pytest.mark.parametrize("sum_quals", [True, False])
def test_three_bams_golden(tmp_path, hip_device, sum_quals):
    M._same(M._run(tmp_path, "device", sum_quals, **KW), M._golden(sum_quals))


@pytest.mark.parametrize("module", ["svtyper_amd.classic", "svtyper_amd.singlesample"])
def test_command_line(tmp_path, hip_device, module):
    out = str(tmp_path / "device.vcf")
    common = ["-i", H.IN_VCF, "-B", H.IN_BAM, "-l", H.LIB_JSON]
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-m", module] + common + ["-o", out, "--reader", "device", "--inflate", "device"], check=True, env=env,
                   cwd=ROOT, timeout=600)
    H.same_vcf(out, H.EXPECTED)


def _worker(rank, world, port, driver, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import test_sharded_drivers as S
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = open(out_path, "w") if rank == 0 else io.StringIO()
    with open(H.IN_VCF) as f:
        if driver == "classic":
            sharded.sv_genotype_sharded(H.IN_BAM, f, out, *S._classic_args(), rank=rank, world=world, **KW)
        else:
            sharded.sso_genotype_sharded(H.IN_BAM, f, out, *S._sso_args(), rank=rank, world=world, **KW)
    if rank == 0:
        out.close()
    sharded.finish()


@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_two_ranks_gloo(tmp_path, hip_device, driver):
    import torch.multiprocessing as mp
    import test_device_reader_drivers as D
    out = str(tmp_path / "out.vcf")
    mp.spawn(_worker, args=(2, D._free_port(), driver, out), nprocs=2, join=True)
    H.same_vcf(out, H.EXPECTED)

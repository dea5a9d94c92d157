"""CSI indexes on the GPU reader routes.  No kernel knows of the index, but the arena planner of both device readers takes its
ranges from it and the device library scan its segment cuts: svt_bam_evidence_device / _device_inflate and
svt_bam_scan_libraries_device on BAMs that carry only a .csi (tests/csicases.py) against the host reader on the same file,
the long contigs against the reference's records (tests/golden/long_contig_sites.json.gz), and both command lines with every
stage on the device.  The same inputs pass on the CPU first: tests/test_csi_index_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import csicases as CC
import libscancases as lc
import test_host_pipeline as H
import walkcases as W
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
ROOT = lc.ROOT


@pytest.fixture(scope="module")
def workdir(hip_device, tmp_path_factory):
    return tmp_path_factory.mktemp("csi_device")


@pytest.fixture(scope="module")
def fixture_input():
    return W.fixture_input()


@pytest.fixture(scope="module")
def long_groups(workdir):
    return CC.long_contig_groups(workdir)


def device_records(sites, sample, nbam, inflate):
    """(offsets, records, skip flags, stats) of the device reader's resident batch, and the host reader's three arrays"""
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    want = nbam.evidence(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, W.header_batch(sample, a[1]), 0, 0, 2,
                                             inflate=inflate)
    off, recs = nr.batch_records(d)
    d.close()
    return (off, recs, skipped, stats), want


def all_zero(by_reason):
    return not any(by_reason.values()) if isinstance(by_reason, dict) else not np.asarray(by_reason).any()


# ------------------------------------------------------------------------------------------ 8. the device readers
@pytest.mark.parametrize("inflate", ["host", "device"])
@pytest.mark.parametrize("shape", [(14, 6), (16, 5)])
def test_fixture_csi_only(workdir, fixture_input, shape, inflate):
    sites, sample, with_bai = fixture_input
    path = CC.csi_only_copy(with_bai.filename, workdir / ("fixture_%d_%d_%s" % (shape + (inflate,))), shape)
    nbam = nr.NativeBam(path)
    assert nbam.index_info() == {"kind": "csi", "min_shift": shape[0], "depth": shape[1]}
    got, want = device_records(sites, sample, nbam, inflate)
    (_, _, _, bai_stats), bai_want = device_records(sites, sample, with_bai, inflate)
    assert len(sites) == 211 and got[3]["n_units"] == 211
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, bai_want)) and len(want[1]) > 5000
    assert got[3]["units_host"] == 0 and all_zero(got[3]["units_host_by_reason"])
    assert bai_stats["units_host"] == 0 and all_zero(bai_stats["units_host_by_reason"])


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_long_contigs(long_groups, inflate):
    import test_geometry_edges as E
    n_units = 0
    for grp, sites, sample, nbam in long_groups:
        assert nbam.index_info() == {"kind": "csi", "min_shift": 14, "depth": 6}
        got, want = device_records(sites, sample, nbam, inflate)
        off, golden = E.golden_unit_records(grp)
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
        assert not got[2].any() and np.array_equal(got[0], off)
        E.assert_records_equal(got[1], golden, "device reader, shift %d" % grp["shift"])
        assert got[3]["units_host"] == 0 and all_zero(got[3]["units_host_by_reason"])
        n_units += got[3]["n_units"]
    assert n_units == 60


# ------------------------------------------------------------------------------------------ 9. the device library scan
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_library_scan_on_csi_cuts(workdir, inflate):
    fixture = nr.NativeBam(CC.csi_only_copy(lc.FIXTURE, workdir / ("scan_fixture_" + inflate), (14, 6)))
    groups = [[rg["ID"] for rg in fixture.header["RG"]]]
    for num_samp in (0, 21277, 1000000):
        for round_bytes in (0, lc.SMALL_ROUND):
            st = lc.compare(fixture, groups, num_samp, round_bytes, route="device", inflate=inflate, expect_reason=lc.WALK)
            assert st["records_walked"] == 42801 and st["segments"] > 1
    src = os.path.join(str(workdir), "short.bam")
    if not os.path.exists(src):
        lc.write_short(src)
    for shape in ((14, 6), (16, 5)):
        short = nr.NativeBam(CC.csi_only_copy(src, workdir / ("scan_short_%d_%d_%s" % (shape + (inflate,))), shape))
        assert short.index_info()["kind"] == "csi"
        for round_bytes in (0, lc.SMALL_ROUND):
            st = lc.compare(short, [["r0"], ["r1"]], 1000000, round_bytes, route="device", inflate=inflate, expect_reason=lc.WALK)
            assert st["records_walked"] == 120000


# ------------------------------------------------------------------------------------------ 10. the command lines
def _command_line(module, path, out, *more):
    r = subprocess.run([sys.executable, "-m", module, "-i", H.IN_VCF, "-B", path, "-o", out, "--reader", "device", "--inflate", "device",
                        "--library-scan", "device"] + list(more), env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("module", ["svtyper_amd.classic", "svtyper_amd.singlesample"])
def test_command_line_with_every_stage_on_the_device(workdir, module):
    """`--reader device --inflate device --library-scan device` on the CSI-only fixture.

    With the library file of the fixture (-l tests/data/NA12878.bam.json) the output is tests/data/example.gt.vcf byte for byte:
    that file was made with it.  Without -l the libraries come from the device scan of the file, and then no index kind gives
    example.gt.vcf -- the scanned libraries are not the JSON's: 49 of its 354 lines differ on the BAI-indexed fixture as well,
    before and after CSI indexes were read -- so that run is held against the same call on the BAI-indexed fixture instead."""
    from svtyper_amd import classic, singlesample
    path = CC.csi_only_copy(lc.FIXTURE, workdir / ("cli_" + module), (14, 6))
    with_l, without_l, bai = (os.path.join(str(workdir), module + tag) for tag in (".l.vcf", ".scan.vcf", ".bai.vcf"))
    _command_line(module, path, with_l, "-l", H.LIB_JSON)
    H.same_vcf(with_l, H.EXPECTED)
    _command_line(module, path, without_l)
    kw = dict(reader="device", inflate="device", library_scan="device")
    with open(H.IN_VCF) as inf, open(bai, "w") as outf:
        if module.endswith("classic"):
            classic.sv_genotype(lc.FIXTURE, inf, outf, 20, 1, 1, 1000000, None, False, None, None, False, None, 1e10, **kw)
        else:
            singlesample.sso_genotype(lc.FIXTURE, inf, outf, 20, 1, 1, 1000000, None, False, None, False, 1000, 1e10, None, 1000, **kw)
    H.same_vcf(without_l, bai)
    assert sum(1 for l in open(without_l) if not l.startswith("#")) == sum(1 for l in open(H.EXPECTED) if not l.startswith("#"))

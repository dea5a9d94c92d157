"""The library scans on the GPU (svt_bam_scan_libraries_device: svt_library_kernel.h, with svt_inflate_kernel for
inflate="device") against svt_bam_scan_library per library: the cases of tests/test_library_walk_host.py, field for field, and
the drivers with library_scan="device"."""
import io
import os
import subprocess
import sys

import pytest

import libscancases as lc
from libscancases import WALK

pytestmark = pytest.mark.gpu
ROOT = lc.ROOT
VCF = os.path.join(ROOT, "tests", "data", "example.vcf")


@pytest.fixture(scope="module")
def native(hip_device):
    from svtyper_amd import native_reads
    return native_reads


@pytest.fixture(scope="module")
def fixture_bam(native):
    b = native.NativeBam(lc.FIXTURE)
    yield b
    b.close()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("libscan_device"))


@pytest.fixture(scope="module")
def synthetic(native, workdir):
    bams = [native.NativeBam(lc.write_synthetic(os.path.join(workdir, "syn%d.bam" % seed), seed)) for seed in (1, 2, 3)]
    yield bams
    for b in bams:
        b.close()


@pytest.mark.parametrize("inflate", ["device", "host"])
@pytest.mark.parametrize("round_bytes", [0, lc.SMALL_ROUND])
def test_fixture(fixture_bam, round_bytes, inflate):
    groups = [[rg["ID"] for rg in fixture_bam.header["RG"]]]
    for num_samp in lc.FIXTURE_NUM_SAMP:
        st = lc.compare(fixture_bam, groups, num_samp, round_bytes, route="device", inflate=inflate, expect_reason=WALK)
        assert st["rounds"] == (1 if round_bytes == 0 else 19) and st["records_walked"] == 42801


def test_fixture_twice_in_one_process(fixture_bam):
    """the tables are filled with integer atomics only: nothing depends on the order in which the wavefronts arrive"""
    runs = [fixture_bam.scan_libraries([["NA12878.S1"]], 0, route="device", round_bytes=rb, ordered=True) for rb in (0, 0, lc.SMALL_ROUND)]
    assert runs[0] == runs[1] == runs[2] and len(runs[0][0][1]) == 2755


@pytest.mark.parametrize("inflate", ["device", "host"])
def test_synthetic_both_inflate_routes(synthetic, inflate):
    for num_samp in (0, 1, 150, 1000000):
        for rb in (0, lc.SMALL_ROUND):
            st = lc.compare(synthetic[0], lc.GROUPS, num_samp, rb, route="device", inflate=inflate, expect_reason=WALK)
            assert st["records_walked"] == 3000
    assert lc.compare(synthetic[0], lc.GROUPS, 0, 0, route="device", inflate=inflate, expect_reason=WALK)["overflow_entries"] == 10


@pytest.mark.parametrize("which", [1, 2])
def test_synthetic_seeds(synthetic, which):
    for num_samp in (0, 150):
        for rb in (0, lc.SMALL_ROUND):
            lc.compare(synthetic[which], lc.GROUPS, num_samp, rb, route="device", expect_reason=WALK)
    lc.compare(synthetic[which], [["r4", "r1"]], 0, lc.SMALL_ROUND, route="device", expect_reason=WALK)
    lc.compare(synthetic[which], [["r3"], [], ["r2", "r0"]], 40, 0, route="device", expect_reason=WALK)


def test_prevalence_stop_and_a_record_without_rg_behind_every_stop(native, workdir):
    b = native.NativeBam(lc.write_short(os.path.join(workdir, "norg_late.bam"), no_rg_at=110000))
    lc.compare(b, [["r0"]], 100, 0, route="device", expect_reason="no_rg")            # in a round that was taken: the host scan answers
    st = lc.compare(b, [["r0"], ["r1"]], 100, lc.SMALL_ROUND, route="device")
    assert st["host_reason"] == "no_rg"                                               # (library r1 never reaches its stops: the whole file is taken)
    st = lc.compare(b, [["r0"]], 100, lc.SMALL_ROUND, route="device", expect_reason=WALK)
    assert st["records_walked"] < 110000
    res = b.scan_libraries([["r0"]], 500, route="device", round_bytes=lc.SMALL_ROUND)
    assert res[0][2:] == (100000, 100000) and sum(res[0][1].values()) == 500
    b.close()


def test_segment_longer_than_a_round(native, workdir):
    b = native.NativeBam(lc.write_short(os.path.join(workdir, "dense.bam"), n=12000, step=1))
    st = lc.compare(b, [["r0"], ["r1"]], 11000, lc.SMALL_ROUND, route="device", expect_reason=WALK)
    assert st["rounds"] >= 3 and st["records_walked"] == 12000
    b.close()


def test_envelope(native, synthetic, workdir):
    recs = lc.synthetic_records(5, n=400, unplaced=0)
    recs[37]["tags"] = [("NM", "C", 1)]
    path = os.path.join(workdir, "norg.bam")
    lc.bamwriter.write_bam(path, lc.HEADER, lc.REFS, recs, block_bytes=3000)
    b = native.NativeBam(path)
    lc.compare(b, lc.GROUPS, 1000000, 0, route="device", expect_reason="no_rg")
    b.close()
    n = lc.capacities()["libraries"] + 1
    lc.compare(synthetic[0], [["r%d" % (k % 6)] if k < 6 else ["x%d" % k] for k in range(n)], 50, 0, route="device", expect_reason="tables")
    native.library_scan_overflow_limit(3)
    try:
        assert lc.compare(synthetic[1], lc.GROUPS, 0, 0, route="device", expect_reason="overflow")["overflow_entries"] > 3
    finally:
        native.library_scan_overflow_limit(0)
    b = native.NativeBam(lc.corrupt_member(os.path.join(workdir, "syn1.bam"), os.path.join(workdir, "corrupt.bam")))
    for inflate in ("device", "host"):
        assert lc.compare(b, lc.GROUPS, 0, 0, route="device", inflate=inflate)["host_reason"] in ("member", "record")
    b.close()


def _run_driver(driver, out_dir, scan, **kw):
    from svtyper_amd import classic, singlesample
    tag = "%s_%s_%s" % (driver, scan, kw.get("inflate", "host"))
    lib_json, out_vcf = os.path.join(out_dir, tag + ".json"), os.path.join(out_dir, tag + ".vcf")
    with open(VCF) as inf, open(out_vcf, "w") as outf:
        if driver == "classic":
            classic.sv_genotype(lc.FIXTURE, inf, outf, 20, 1, 1, 1000000, lib_json, False, None, None, False, None, 1e10, library_scan=scan, **kw)
        else:
            singlesample.sso_genotype(lc.FIXTURE, inf, outf, 20, 1, 1, 1000000, lib_json, False, None, False, 1000, 1e10, None, 1000,
                                      library_scan=scan, **kw)
    strip = lambda text: b"\n".join(l for l in text.split(b"\n") if not l.startswith(b"##fileDate"))
    return open(lib_json, "rb").read(), strip(open(out_vcf, "rb").read())


@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_drivers_with_the_device_scan(native, workdir, driver):
    """no library file yet: the scan builds it.  The JSON written and the VCF are the host scan's, byte for byte."""
    host_json, host_vcf = _run_driver(driver, workdir, "host")
    dev_json, dev_vcf = _run_driver(driver, workdir, "device")
    assert dev_json == host_json and len(host_json) > 10000
    assert dev_vcf == host_vcf and host_vcf.count(b"\n") > 200
    # the device reader with its members inflated on the GPU: the scan's members are inflated there too
    inf_json, inf_vcf = _run_driver(driver, workdir, "device", reader="device", inflate="device")
    assert inf_json == host_json and inf_vcf == host_vcf


@pytest.mark.parametrize("module", ["svtyper_amd.classic", "svtyper_amd.singlesample"])
def test_command_lines_accept_library_scan(native, workdir, module):
    out = os.path.join(workdir, module + ".vcf")
    lib_json = os.path.join(workdir, module + ".json")
    code = "import sys; from %s import main; sys.exit(main())" % module
    r = subprocess.run([sys.executable, "-c", code, "-B", lc.FIXTURE, "-i", VCF, "-o", out, "-l", lib_json, "--library-scan", "device"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.getsize(lib_json) > 10000 and os.path.getsize(out) > 10000

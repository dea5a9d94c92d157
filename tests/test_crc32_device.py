"""BGZF CRC32 verification on the GPU: svt_crc32_kernel (svtyper_amd/csrc/svt_crc32_kernel.h) against zlib.crc32,
svt_bgzf_inflate_device_verified against the host function, and verify="crc32" through reader="device", inflate="device" and
library_scan="device" on the fixture and on the damaged copy of tests/crccases.py."""
import os
import random
import zlib

import numpy as np
import pytest

import crccases as cc
import inflatecases as ic
import test_host_pipeline as H
from svtyper_amd import classic, hip, native_reads as nr, singlesample

pytestmark = pytest.mark.gpu
CRC = nr.INFLATE_CRC
MISMATCH = r"BGZF block at offset %d: CRC32 mismatch \(stored 0x[0-9a-f]{8}, computed 0x[0-9a-f]{8}\)"


def test_crc32_device_is_zlibs_on_the_length_and_content_grid(hip_device):
    members, off = cc.grid()
    got = nr.bgzf_crc32(b"".join(members), off, device=0)
    want = np.array([zlib.crc32(m) for m in members], np.uint32)
    bad = [(k, len(members[k]), hex(int(got[k])), hex(int(want[k]))) for k in np.nonzero(got != want)[0]]
    assert not bad, bad[:8]


def test_crc32_device_on_4096_members_of_mixed_lengths_twice(hip_device):
    data, off = cc.mixed(4096)
    first = nr.bgzf_crc32(data, off, device=0)
    second = nr.bgzf_crc32(data, off, device=0)
    assert (first == second).all()
    assert first.tolist() == [zlib.crc32(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]


def test_inflate_device_verified_gives_the_host_functions_statuses_and_the_true_bytes(hip_device):
    rnd = random.Random(5)
    clean = cc.with_true_crc(ic.zlib_members() + ic.token_members() + ic.bam_members([cc.FIXTURE])[:12])
    bad = ic.corruption_corpus(ic.bam_members([cc.FIXTURE]))[::7] + ic.token_bad_members()
    small = cc.with_true_crc([cc.sized_member(rnd, n) for n in (1, 63, 65, 65535)])
    entries = []
    for k, e in enumerate(clean):
        entries.append((e[0], cc.flip_trailer_bit(e[1], rnd.randrange(32))) if k % 3 == 1 else e)
    for k, e in enumerate(clean[:8]):                          # a flipped trailer between clean members of ISIZE 1, 63, 65 and 65 535
        entries += [small[k % 4], (e[0] + "/flipped", cc.flip_trailer_bit(e[1], rnd.randrange(32))), small[(k + 1) % 4]]
    entries += bad
    data, block_off, out_off = ic.layout([m for _l, m in entries])
    h_out, h_status = nr.bgzf_inflate(data, block_off, out_off, verified=True)
    d_out, d_status = nr.bgzf_inflate(data, block_off, out_off, device=0, verified=True)
    diff = [(entries[k][0], int(h_status[k]), int(d_status[k])) for k in np.nonzero(h_status != d_status)[0]]
    assert not diff, diff[:8]
    assert (d_status == CRC).sum() >= len(clean) // 3 + 8 and (d_status == 0).sum() > 50
    for k, (label, m) in enumerate(entries):
        if d_status[k] == 0:
            assert d_out[int(out_off[k]):int(out_off[k + 1])].tobytes() == zlib.decompress(ic.split_member(m)[0], -15), label
    _o, plain = nr.bgzf_inflate(data, block_off, out_off, device=0)       # the plain entry point keeps its verdicts
    assert (plain == np.where(d_status == CRC, 0, d_status)).all()


KW = dict(reader="device", inflate="device", verify="crc32")


@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_device_reader_with_verify_on_the_fixture(tmp_path, hip_device, driver):
    out = str(tmp_path / "out.vcf")
    stats = {}
    if driver == "classic":
        H.run_classic(out, None, stats=stats, **KW)
    else:
        H.run_sso(out, None, None, stats=stats, **KW)
    H.same_vcf(out, H.EXPECTED)
    print(stats["verify"], stats["device_reader"]["inflate"])
    assert stats["verify"]["members_verified"] == stats["device_reader"]["inflate"]["blocks_inflated"] > 0
    assert stats["verify"]["members_failed"] == 0 and stats["verify"]["device_crc_s"] > 0


@pytest.fixture(scope="module")
def damaged(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("crc") / "damaged.bam")
    return path, cc.damaged_fixture(path)


def _run(driver, bam, out, lib_json=H.LIB_JSON, **kw):
    with open(H.IN_VCF) as inf, open(out, "w") as outf:
        if driver == "classic":
            classic.sv_genotype(bam, inf, outf, 20, 1, 1, 1000000, lib_json, False, None, None, False, None, 1e10, **kw)
        else:
            singlesample.sso_genotype(bam, inf, outf, 20, 1, 1, 1000000, lib_json, False, None, False, 1000, 1e10, None, 1000, **kw)


@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_device_reader_with_verify_on_the_damaged_copy(tmp_path, hip_device, damaged, driver):
    path, offset = damaged
    out = str(tmp_path / "on.vcf")
    with pytest.raises(hip.SvtyperHipError, match=MISMATCH % offset):
        _run(driver, path, out, **KW)
    assert not [l for l in open(out) if not l.startswith("#")]      # no VCF body
    out = str(tmp_path / "off.vcf")
    _run(driver, path, out, reader="device", inflate="device")      # verify off: accepted, as before
    assert sum(1 for l in open(out) if not l.startswith("#")) > 200


@pytest.mark.parametrize("inflate", ["device", "host"])
def test_device_library_scan_with_verify(tmp_path, hip_device, damaged, inflate):
    path, offset = damaged
    reader = "device" if inflate == "device" else "native"
    host_json = str(tmp_path / "host.json")
    _run("sso", cc.FIXTURE, str(tmp_path / "host.vcf"), host_json, reader="native", library_scan="host")
    dev_json = str(tmp_path / "dev.json")
    _run("sso", cc.FIXTURE, str(tmp_path / "dev.vcf"), dev_json, reader=reader, inflate=inflate, library_scan="device", verify="crc32")
    assert open(dev_json, "rb").read() == open(host_json, "rb").read() and os.path.getsize(host_json) > 10000
    with pytest.raises(hip.SvtyperHipError, match=MISMATCH % offset):
        _run("sso", path, str(tmp_path / "bad.vcf"), str(tmp_path / "bad.json"), reader=reader, inflate=inflate, library_scan="device", verify="crc32")
    # the scan itself: the walk hands the file to the host scan because of the member, and that scan reports it
    b = nr.NativeBam(path, verify=True)
    with pytest.raises(hip.SvtyperHipError, match=MISMATCH % offset):
        b.scan_libraries([[rg["ID"] for rg in b.header["RG"]]], 1000000, route="device", inflate=inflate)
    assert b.library_scan_stats["host_reason"] == "member"
    b.close()


def test_device_library_scan_with_verify_over_many_rounds(hip_device, damaged):
    """the device side of a round's members keeps its buffers and the CRC tables from round to round: verify on at the smallest
    round size, where the fixture takes 19 rounds instead of one"""
    import libscancases as lc
    b = nr.NativeBam(cc.FIXTURE, verify=True)
    groups = [[rg["ID"] for rg in b.header["RG"]]]
    want = lc.host_scan(b, groups, 1000000)
    got = b.scan_libraries(groups, 1000000, route="device", inflate="device", round_bytes=lc.SMALL_ROUND, ordered=True)
    st, vs = b.library_scan_stats, nr.verify_stats()
    print(st, vs)
    assert got == want and st["host_reason"] is None
    assert st["rounds"] > 1
    assert vs["members_verified"] == st["members_inflated"] > 0 and vs["members_failed"] == 0
    b.close()
    path, offset = damaged
    b = nr.NativeBam(path, verify=True)
    with pytest.raises(hip.SvtyperHipError, match=MISMATCH % offset):
        b.scan_libraries(groups, 1000000, route="device", inflate="device", round_bytes=lc.SMALL_ROUND)
    assert b.library_scan_stats["host_reason"] == "member"
    b.close()

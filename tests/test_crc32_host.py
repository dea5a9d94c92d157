"""BGZF CRC32 verification without a GPU: the one-source CRC (svtyper_amd/csrc/svt_crc32.h) on the host against zlib.crc32,
svt_bgzf_inflate_host_verified on the inflate corpus, and verify="crc32" through the host routes -- the C++ reader, the Python
reader, the open-range walk and the library walk -- on the fixture and on a copy of it with one damaged member that still
inflates to ISIZE bytes."""
import os
import random
import zlib

import numpy as np
import pytest

import crccases as cc
import inflatecases as ic
import libscancases as lc
import test_host_pipeline as H
from svtyper_amd import classic, hip, native_reads as nr, singlesample

CRC = nr.INFLATE_CRC


def test_crc32_host_is_zlibs_on_the_length_and_content_grid():
    members, off = cc.grid()
    got = nr.bgzf_crc32(b"".join(members), off)
    want = np.array([zlib.crc32(m) for m in members], np.uint32)
    bad = [(k, len(members[k]), hex(int(got[k])), hex(int(want[k]))) for k in np.nonzero(got != want)[0]]
    assert not bad, bad[:8]
    assert got[-3] != got[-2] and got[-3] != got[-1]           # (the last byte alone, the first byte alone)


def test_crc32_host_on_many_members_of_mixed_lengths_and_bad_arguments():
    data, off = cc.mixed()
    got = nr.bgzf_crc32(data, off)
    assert got.tolist() == [zlib.crc32(data[int(a):int(b)]) for a, b in zip(off[:-1], off[1:])]
    assert nr.bgzf_crc32(b"", np.zeros(1, np.uint64)).shape == (0,)
    with pytest.raises(hip.SvtyperHipError, match="65536"):
        nr.bgzf_crc32(bytes(70000), np.array([0, 65537], np.uint64))
    with pytest.raises(hip.SvtyperHipError, match="decrease"):
        nr.bgzf_crc32(bytes(100), np.array([0, 50, 40], np.uint64))


@pytest.fixture(scope="module")
def corpus():
    clean = cc.with_true_crc(ic.zlib_members() + ic.token_members() + ic.bam_members([cc.FIXTURE])[:12])
    bad = ic.corruption_corpus(ic.bam_members([cc.FIXTURE]))[::7] + ic.token_bad_members()
    return clean, bad


def test_inflate_host_verified_on_the_corpus(corpus):
    clean, bad = corpus
    data, block_off, out_off = ic.layout([m for _l, m in clean])
    out, status = nr.bgzf_inflate(data, block_off, out_off, verified=True)
    assert not status.any(), [(clean[k][0], int(status[k])) for k in np.nonzero(status)[0]][:8]
    # one trailer CRC bit flipped in every third member: SVT_INFLATE_CRC there, 0 elsewhere; the plain entry point sees nothing
    rnd = random.Random(3)
    flipped = [(label, cc.flip_trailer_bit(m, rnd.randrange(32)) if k % 3 == 1 else m) for k, (label, m) in enumerate(clean)]
    data, block_off, out_off = ic.layout([m for _l, m in flipped])
    out, status = nr.bgzf_inflate(data, block_off, out_off, verified=True)
    assert status.tolist() == [CRC if k % 3 == 1 else 0 for k in range(len(flipped))]
    for k, (label, m) in enumerate(flipped):                   # (the bytes of a member whose CRC differs are the inflated ones all the same)
        assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == zlib.decompress(ic.split_member(m)[0], -15), label
    _out, plain = nr.bgzf_inflate(data, block_off, out_off)
    assert not plain.any()
    # the decode verdict comes first: every bad stream keeps the status it has without verify
    data, block_off, out_off = ic.layout([m for _l, m in bad])
    _o, s_plain = nr.bgzf_inflate(data, block_off, out_off)
    _o, s_verified = nr.bgzf_inflate(data, block_off, out_off, verified=True)
    keeps = (s_verified == s_plain) | ((s_plain == 0) & (s_verified == CRC))       # (a flip that still inflates: its crc was written as 0)
    assert keeps.all() and (s_plain != 0).sum() > 50
    assert ((s_plain != 0) == (s_verified != 0))[s_plain != 0].all() and not (s_verified[s_plain != 0] == CRC).any()


def test_get_verify_is_0_on_a_fresh_handle_and_the_property_sets_it():
    b = nr.NativeBam(cc.FIXTURE)
    assert b._L.svt_bam_get_verify(b._h) == 0 and b.verify is False
    b.verify = True
    assert b._L.svt_bam_get_verify(b._h) == 1 and b.verify is True
    b.verify = False
    assert b.verify is False
    assert nr.NativeBam(cc.FIXTURE, verify=True).verify is True
    b.close()


@pytest.mark.parametrize("driver", ["classic", "sso"])
@pytest.mark.parametrize("reader", ["native", "python"])
def test_clean_fixture_with_verify_on(tmp_path, driver, reader):
    out = str(tmp_path / "out.vcf")
    stats = {}
    if driver == "classic":
        H.run_classic(out, H.oracle_engine, reader=reader, verify="crc32", stats=stats)
    else:
        H.run_sso(out, H.oracle_engine, None, reader=reader, verify="crc32", stats=stats)
    H.same_vcf(out, H.EXPECTED)
    print(stats["verify"])
    assert stats["verify"]["members_verified"] > 0 and stats["verify"]["members_failed"] == 0


@pytest.fixture(scope="module")
def damaged(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("crc") / "damaged.bam")
    return path, cc.damaged_fixture(path)


def _run(driver, bam, out, **kw):
    with open(H.IN_VCF) as inf, open(out, "w") as outf:
        if driver == "classic":
            classic.sv_genotype(bam, inf, outf, 20, 1, 1, 1000000, H.LIB_JSON, False, None, None, False, None, 1e10, engine=H.oracle_engine, **kw)
        else:
            singlesample.sso_genotype(bam, inf, outf, 20, 1, 1, 1000000, H.LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                      engine=H.oracle_engine, **kw)


@pytest.mark.parametrize("driver", ["classic", "sso"])
@pytest.mark.parametrize("reader", ["native", "python"])
def test_damaged_member_is_accepted_with_verify_off_and_raises_with_verify_on(tmp_path, damaged, driver, reader):
    path, offset = damaged
    out = str(tmp_path / "off.vcf")
    _run(driver, path, out, reader=reader)                     # runs to completion: nobody looks at the CRC
    assert sum(1 for l in open(out) if not l.startswith("#")) > 200
    out = str(tmp_path / "on.vcf")
    with pytest.raises(IOError if reader == "python" else hip.SvtyperHipError, match=r"BGZF block at offset %d: CRC32 mismatch \(stored 0x[0-9a-f]{8}, computed 0x[0-9a-f]{8}\)" % offset):
        _run(driver, path, out, reader=reader, verify="crc32")


def test_walks_flag_the_units_over_the_damaged_member(damaged):
    """svt_bam_evidence_walk_host / _walk_open_host have no fallback: with verify on the units over the member come back flagged
    SVT_WALK_RANGE, as over a member that does not inflate; with verify off nothing is flagged"""
    import walkcases as W
    path, _offset = damaged
    sites, sample, _nbam = W.fixture_input()
    b = nr.NativeBam(path)
    win, bps, rgs, rg_lib, flank = W.unit_arrays(sites, sample, b, nr.COUNT_SSO)
    a = (win, bps, rgs, rg_lib, 1000, nr.COUNT_SSO, flank, 20, 3, 2)
    for entry in (b.evidence_walk_host, b.evidence_walk_open_host):
        b.verify = False
        assert not entry(*a)[3].any()
        b.verify = True
        flagged = entry(*a)[3]
        assert flagged.any() and set(flagged[flagged != 0].tolist()) == {2}
        assert nr.verify_stats()["members_failed"] >= 1
    b.close()


def test_library_walk_on_the_host_ends_in_the_error(damaged):
    path, offset = damaged
    b = nr.NativeBam(path)
    rgs = [[rg["ID"] for rg in b.header["RG"]]]
    clean = nr.NativeBam(cc.FIXTURE, verify=True)
    want = clean.scan_libraries(rgs, 1000000, route="walk_host")
    assert clean.library_scan_stats["host_reason"] is None
    assert nr.verify_stats()["members_verified"] == clean.library_scan_stats["members_inflated"] and nr.verify_stats()["members_failed"] == 0
    got = b.scan_libraries(rgs, 1000000, route="walk_host")   # verify off: answers as today (one bit of a record's bytes differs)
    assert b.library_scan_stats["host_reason"] is None and got[0][3] == want[0][3]
    b.verify = True
    with pytest.raises(hip.SvtyperHipError, match="BGZF block at offset %d: CRC32 mismatch" % offset):
        b.scan_libraries(rgs, 1000000, route="walk_host")
    assert b.library_scan_stats["host_reason"] == "member"
    with pytest.raises(hip.SvtyperHipError, match="BGZF block at offset %d: CRC32 mismatch" % offset):
        b.scan_library(rgs[0], 1000000)
    assert b.verify_stats["members_failed"] >= 2
    b.close()
    clean.close()


def test_library_walk_on_the_host_with_verify_over_many_rounds(damaged):
    """the host twin of the device scan's many-rounds case: svt_bam_scan_libraries_walk_host at the smallest round size"""
    b = nr.NativeBam(cc.FIXTURE, verify=True)
    groups = [[rg["ID"] for rg in b.header["RG"]]]
    want = lc.host_scan(b, groups, 1000000)
    got = b.scan_libraries(groups, 1000000, route="walk_host", round_bytes=lc.SMALL_ROUND, ordered=True)
    st, vs = b.library_scan_stats, nr.verify_stats()
    assert got == want and st["host_reason"] is None
    assert st["rounds"] > 1
    assert vs["members_verified"] == st["members_inflated"] > 0 and vs["members_failed"] == 0
    b.close()
    path, offset = damaged
    b = nr.NativeBam(path, verify=True)
    with pytest.raises(hip.SvtyperHipError, match="BGZF block at offset %d: CRC32 mismatch" % offset):
        b.scan_libraries(groups, 1000000, route="walk_host", round_bytes=lc.SMALL_ROUND)
    assert b.library_scan_stats["host_reason"] == "member"
    b.close()

"""The tag grammar and the CIGAR operation classes of svtyper_amd/csrc/svt_record_rules.h in the three kernels that decode BAM
records -- svt_evidence_kernel, svt_evidence_deep_kernel and svt_library_kernel -- over the corpus of tests/grammarcases.py.
The comparison is the host reader's bytes, as in the other device tests; what makes it a check of the grammar is that
tests/test_record_grammar_host.py pins those bytes, for these very inputs, to the Python reader and to grammarcases.spec_tags,
neither of which passes through rr::walk_tags.  Well-formed records only, and no unit and no scan may fall back to the host:
a kernel that loses its way in a tag area has to show here and not in a fallback counter.  One workgroup per tier, one scan of
one round and one of several."""
import pytest

import grammarcases as G
import libscancases as lc
import test_device_inflate_reader as I
import test_device_reader as R
from svtyper_amd import evidence as ev, native_reads as nr

pytestmark = pytest.mark.gpu
FLAGS = (0, ev.FLAG_SSO_ASSOCIATION | ev.FLAG_RESULT96)
MODES = (nr.COUNT_CLASSIC, nr.COUNT_SSO)


def test_lds_tier(tmp_path, hip_device):
    """svt_evidence_kernel: records and offsets in HBM are the host reader's, genotype results are those on svt_batch_create's
    batch (test_device_reader._compare)"""
    sites, sample, nbam = G.evidence_input(tmp_path)
    for mode in MODES:
        stats, want = R._compare(sites, sample, nbam, mode, None, flags=FLAGS)
        assert stats["units_host"] == 0 and stats["units_host_by_reason"] == {} and stats["deep"]["units_deep"] == 0
        assert len(want[1]) >= len(G.evidence_records()) and not want[2].any()


def test_deep_tier(tmp_path, hip_device):
    """svt_evidence_deep_kernel: the same for a unit of G.N_DEEP kept reads"""
    sites, sample, nbam = G.deep_input(tmp_path)
    for mode in MODES:
        stats, want = R._compare(sites, sample, nbam, mode, None, flags=FLAGS)
        assert stats["units_host"] == 0 and stats["units_host_by_reason"] == {}
        assert stats["deep"]["units_deep"] == 1 and stats["deep"]["reads_deep"] == G.N_DEEP <= len(want[1])


@pytest.mark.parametrize("inflate", ["device", "host"])
def test_library_scan(tmp_path, hip_device, inflate):
    """svt_library_kernel: every decoration in front of RG; the walk answers itself (host_reason is None) in one round and in
    several"""
    b = nr.NativeBam(G.library_input(str(tmp_path / "grammar_lib.bam")))
    try:
        for num_samp in (0, 150):
            for rb in (0, lc.SMALL_ROUND):
                st = lc.compare(b, lc.GROUPS, num_samp, rb, route="device", inflate=inflate, expect_reason=lc.WALK)
                assert st["host_reason"] is None and st["records_walked"] == G.N_LIBRARY and (st["rounds"] > 1) == (rb != 0)
    finally:
        b.close()


def test_device_inflate_route(tmp_path, hip_device):
    """the decorated reads once through reader="device", inflate="device" (test_device_inflate_reader._compare)"""
    sites, sample, nbam = G.evidence_input(tmp_path)
    stats, want = I._compare(sites, sample, nbam, nr.COUNT_SSO, None, flags=(ev.FLAG_SSO_ASSOCIATION,))
    assert stats["units_host"] == 0 and stats["inflate"]["blocks_failed"] == 0 and stats["inflate"]["blocks_inflated"] > 0
    assert len(want[1]) >= len(G.evidence_records())

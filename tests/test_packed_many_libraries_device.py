"""Packed evidence of more than 256 libraries on the GPU (svt_packed_kernel<kLibsInHbm>): the pass over the packed slots
returns the bytes of the pass over the canonical records of the same batch, and both agree with the oracle -- at the first
batch past the old limit, past the short switch's field, at library 65 535, with a unit's records alternating across the
short / wide boundary, on a resident batch run twice and through svt_genotype_packed_from_records."""
import numpy as np
import pytest

from svtyper_amd import evidence as ev

import manylibcases


def _oracle(batch, flags):
    from oracle import c_oracle
    return c_oracle.genotype_batch(batch, flags=flags)


def _wide_switches(p, n_units):
    """wide library switches in the PAIR streams of packed evidence (the other two streams of a unit hold no half-word
    entries): a pair of half-words starts at an even one, so 0x8000 there is a wide switch and nothing else"""
    half = p.slots().view(np.uint16).reshape(-1, 8)
    so = p.slot_offset()
    count = 0
    for u in range(n_units):
        h = half[int(so[3 * u]):int(so[3 * u + 1])].reshape(-1)
        k = 0
        while k < len(h):
            if int(h[k]) == 0x8000:
                count += 1
            k += 2 if int(h[k]) & 0x8000 else 1
    return count


def _packed_equals_canonical(batch, flags, device):
    from svtyper_amd import hip
    from test_hip_parity import assert_parity
    with hip.PackedEvidence(batch, many_libraries=True) as p:
        assert _wide_switches(p, min(batch.n_units, 400)) > 0, "no wide switch in the pair streams"
        got = hip.genotype_packed(p, device=device, flags=flags)
    canon = hip.genotype_batch(batch, device=device, flags=flags)
    assert got.rec.tobytes() == canon.rec.tobytes(), "packed pass differs from the pass over the canonical records"
    assert_parity(got, _oracle(batch, flags))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("sso", [0, ev.FLAG_SSO_ASSOCIATION])
@pytest.mark.parametrize("n_libs", [257, 300, 4200])
def test_packed_pass_of_many_libraries(hip_device, fixture_library, n_libs, sso):
    """2 000 units of ~20 records: 257 (one library takes the wide switch), 300 (150 samples x 2 and more), 4 200 (beyond
    what the short switch's twelve bits could name)"""
    got = _packed_equals_canonical(manylibcases.many_libraries(fixture_library, n_libs, 2000), sso, hip_device)
    assert (got.gt >= 0).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("sso", [0, ev.FLAG_SSO_ASSOCIATION])
def test_highest_library(hip_device, fixture_library, sso):
    """65 536 libraries, the units name 0..2 and 65 533..65 535"""
    batch = manylibcases.highest_library(fixture_library)
    assert int((batch.records["flags"] >> ev.REC_LIB_SHIFT).max()) == 65535
    _packed_equals_canonical(batch, sso, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("sso", [0, ev.FLAG_SSO_ASSOCIATION])
def test_records_alternate_across_the_switch_boundary(hip_device, fixture_library, sso):
    """library 255 / 256 (and 254 / 257) record by record inside every unit: a short and a wide switch in turn, in every
    alignment, in more than one workgroup"""
    batch = manylibcases.interleaved_across_the_boundary(fixture_library)
    assert batch.n_units > 256
    _packed_equals_canonical(batch, sso, hip_device)


@pytest.mark.gpu
def test_resident_batch_and_from_records(hip_device, fixture_library):
    """svt_batch_create_packed + two passes; svt_genotype_packed_from_records -- the plain sequence (a small batch) and the
    overlapped one (ranges of units), with 96-byte device records too"""
    from svtyper_amd import hip
    batch = manylibcases.many_libraries(fixture_library, 300, 2000)
    want = hip.genotype_batch(batch, device=hip_device).rec.tobytes()
    with hip.PackedEvidence(batch, many_libraries=True) as p, hip.DeviceBatch.from_packed(p, hip_device) as d:
        assert d.layout_name() == "packed"
        d.genotype(sync=True)
        first = d.results().rec.tobytes()
        d.genotype(sync=True)
        assert d.results().rec.tobytes() == first == want
    assert hip.genotype_packed_from_records(batch, hip_device, 0).rec.tobytes() == want
    big = manylibcases.many_libraries(fixture_library, 300, 40_000)          # above the pipeline's minimum: encoder ahead of the wire
    sso96 = ev.FLAG_SSO_ASSOCIATION | ev.FLAG_RESULT96
    want_big = {flags: hip.genotype_batch(big, device=hip_device, flags=flags & ev.FLAG_SSO_ASSOCIATION).rec.tobytes() for flags in (0, sso96)}
    for flags in (0, sso96):
        assert hip.genotype_packed_from_records(big, hip_device, flags).rec.tobytes() == want_big[flags]
    with hip.PackedEvidence(big, many_libraries=True) as p:                    # svt_genotype_packed, pipelined by unit ranges
        assert hip.genotype_packed(p, device=hip_device, flags=sso96).rec.tobytes() == want_big[sso96]

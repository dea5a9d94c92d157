"""svt_bam_evidence_walk_host -- the one-source evidence walk (svtyper_amd/csrc/svt_evidence_walk.h) over host memory, no GPU, no
fallback -- against the shipped host reader svt_bam_evidence: rec_offset, records and skipped byte for byte for every unit that is
not flagged; no unit of the listed inputs is flagged; a unit built to leave the envelope is flagged with its reason and empty.
Per-unit maxima of kept reads measured with this entry (the tests print them): fixture 617 without max_reads (300 / 240 under the
limits of its cases), three-BAM golden inputs 565, fake-read BAMs 52; the capacity is 1024."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import walkcases as W
from svtyper_amd import hip, native_reads as nr

ROOT = os.path.dirname(W.HERE)


def _both(sites, sample, nbam, mode, max_reads, threads=2):
    a = W.unit_arrays(sites, sample, nbam, mode)
    want = nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, threads)
    got = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, threads)
    return want, got


def _assert_equal(want, got):
    assert not got[3].any(), "flagged units: %s" % np.bincount(got[3])
    assert np.array_equal(got[2], want[2]), "skip flags differ"
    assert np.array_equal(got[0], want[0]), "record counts differ"
    assert got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("mode,max_reads", [(nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 120), (nr.COUNT_CLASSIC, 150)])
def test_fixture_equals_the_host_reader(mode, max_reads):
    sites, sample, nbam = W.fixture_input()
    want, got = _both(sites, sample, nbam, mode, max_reads)
    _assert_equal(want, got)
    print("kept reads per unit: max %d" % int(got[4].max()))
    assert int(got[4].max()) <= nr.walk_capacities()["reads"]
    assert len(want[1]) > 5000 or want[2].any()


@pytest.mark.parametrize("seed", W.SYNTHETIC_SEEDS)
@pytest.mark.parametrize("sa_first", [False, True])
def test_synthetic_bams_equal_the_host_reader(tmp_path, seed, sa_first):
    sites, sample, nbam = W.synthetic_input(tmp_path, seed, sa_first=sa_first, tied_names=(seed % 2 == 0))
    for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_CLASSIC, 90), (nr.COUNT_SSO, 200)):
        want, got = _both(sites, sample, nbam, mode, max_reads)
        _assert_equal(want, got)
    assert (want[1]["seq_l"] | want[1]["clip_l"] | want[1]["seq_r"] | want[1]["clip_r"]).any() or want[2].all()


def test_fake_read_bams_equal_the_host_reader(tmp_path):
    n = 0
    for sites, sample, nbam in W.fake_inputs(tmp_path):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 30), (nr.COUNT_CLASSIC, 25)):
            want, got = _both(sites, sample, nbam, mode, max_reads)
            _assert_equal(want, got)
        n += len(want[1])
        print("kept reads per unit: max %d" % int(got[4].max()))
    assert n > 1000


def test_three_bam_golden_inputs_equal_the_host_reader(tmp_path):
    for sites, sample, nbam in W.three_bam_inputs(tmp_path):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000)):
            want, got = _both(sites, sample, nbam, mode, max_reads)
            _assert_equal(want, got)
            print("kept reads per unit: max %d" % int(got[4].max()))
        assert len(want[1]) > 50


N_BOUNDARY = 37


@pytest.mark.parametrize("mode", [nr.COUNT_CLASSIC, nr.COUNT_SSO])
def test_max_reads_boundaries_skip_and_do_not_flag(tmp_path, mode):
    """A window with exactly N countable, kept reads.  count_mode 1 skips when the window's count exceeds max_reads: N - 1
    skips, N and N + 1 keep.  count_mode 0 skips when a kept read's index in the fetch (0 .. N - 1) exceeds max_reads: N - 2
    skips, N - 1, N and N + 1 keep.  Skipped units are skipped, never flagged, and equal the host reader's either way."""
    sites, sample, nbam = W.boundary_input(tmp_path, N_BOUNDARY)
    first_kept = N_BOUNDARY if mode == nr.COUNT_SSO else N_BOUNDARY - 1
    for limit in (N_BOUNDARY - 2, N_BOUNDARY - 1, N_BOUNDARY, N_BOUNDARY + 1):
        want, got = _both(sites, sample, nbam, mode, limit)
        _assert_equal(want, got)
        assert bool(got[2][0]) == (limit < first_kept), "max_reads %d" % limit
        assert (len(got[1]) == 0) == (limit < first_kept)
        if limit >= first_kept:
            assert int(got[4][0]) == N_BOUNDARY


@pytest.mark.parametrize("case", ["reads", "name", "cigar", "sa_entries", "no_rg", "unknown_rg", "malformed_sa"])
def test_units_outside_the_envelope_are_flagged_and_empty(tmp_path, case):
    records, reason, host_fails = W.envelope_cases(nr.walk_capacities())[case]
    sample, nbam = W.open_sample(W.write_case(tmp_path, case, records), W.INFO)
    a = W.unit_arrays([{"breakpoint": W.SITE}], sample, nbam, nr.COUNT_SSO)
    got = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert nr.WALK_REASONS[int(got[3][0])] == reason
    assert int(got[0][-1]) == 0 and len(got[1]) == 0 and not got[2].any()
    if host_fails:
        with pytest.raises(hip.SvtyperHipError):
            nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    else:
        assert len(nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)[1]) > 0


def test_truncated_last_record_is_flagged(tmp_path):
    """the BGZF block that holds the last record is cut short: the unit is flagged (range), nothing is read out of range"""
    sites, sample, nbam = W.truncated_input(tmp_path)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    got = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert nr.WALK_REASONS[int(got[3][0])] == "range" and len(got[1]) == 0


def test_a_tag_that_runs_over_the_record_is_malformed(tmp_path):
    """a B array whose count reaches beyond the record's end, behind RG: flagged, as everything the host reader does not take as is"""
    import struct
    bad = ("XB", "raw", b"XBBi" + struct.pack("<I", 1000) + b"\0" * 8)
    records = [W._read("ok%d" % k, 50_000 + k) for k in range(3)] + [W._read("t", 50_010, tags=[("RG", "Z", "rg"), bad])]
    sample, nbam = W.open_sample(W.write_case(tmp_path, "overrun", records), W.INFO)
    a = W.unit_arrays([{"breakpoint": W.SITE}], sample, nbam, nr.COUNT_SSO)
    got = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert nr.WALK_REASONS[int(got[3][0])] == "malformed" and len(got[1]) == 0


def test_abi_of_the_new_structs(tmp_path):
    """the C view of svt_evidence_device_stats and the reason / capacity macros against the ctypes binding"""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svtyper_reads.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(svt_evidence_device_stats), '
                   'offsetof(svt_evidence_device_stats, units_host_by_reason), offsetof(svt_evidence_device_stats, n_records), '
                   'offsetof(svt_evidence_device_stats, batch_create_s), SVT_WALK_N_REASONS, SVT_WALK_MAPQ, SVT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, by_reason, n_records, last, n_reasons, mapq, abi = (int(x) for x in subprocess.check_output([str(exe)]).split())
    S = nr._DeviceStats
    assert (size, by_reason, n_records, last) == (C.sizeof(S), S.units_host_by_reason.offset, S.n_records.offset, S.batch_create_s.offset)
    assert n_reasons == 11 and nr.WALK_REASONS[mapq] == "mapq" and max(nr.WALK_REASONS) == n_reasons - 1
    assert abi == hip.ABI_VERSION == 19
    L = hip.load()
    assert all(hasattr(L, f) for f in ("svt_bam_evidence_walk_host", "svt_bam_evidence_device", "svt_debug_batch_records"))

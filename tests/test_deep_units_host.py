"""The deep tier of the evidence walk on the CPU: units of more than 1 024 and up to 16 384 kept reads through
svt_bam_evidence_walk_host and svt_bam_evidence_walk_open_host (svt_evidence_walk.h: DeepScratch + Tables<uint32_t>, tiles and
merges instead of the rank sort) against the shipped host reader svt_bam_evidence -- rec_offset, records and skipped byte for byte.
A unit beyond 16 384 reads is flagged `reads` with its true number of kept reads and comes back empty."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import deepcases as D
import walkcases as W
from svtyper_amd import hip, native_reads as nr
from test_sanitizers import ROOT, asan_env  # noqa: F401  (the module-scoped fixture that builds the instrumented library)

ENTRIES = ["evidence_walk_host", "evidence_walk_open_host"]


def _compare(sites, sample, nbam, mode, max_reads, entry):
    a, want = D.host_reader(sites, sample, nbam, mode, max_reads)
    got = D.walk(nbam, a, mode, max_reads, entry)
    print("%s mode %d max_reads %s: kept reads %s flagged %s records %d" % (entry, mode, max_reads, got[4].tolist(), got[3].tolist(), len(got[1])))
    return want, got


def _assert_all_equal(want, got):
    assert not got[3].any(), "flagged units: %s" % got[3].tolist()
    assert np.array_equal(got[0], want[0]), "record counts differ"
    D.assert_units_equal(want, got[0], got[1], got[2])


def test_capacities():
    cap = nr.walk_capacities()
    assert (cap["reads"], cap["reads_lds"]) == (D.DEEP, D.LDS) == (16384, 1024)
    assert nr.WALK_CAPACITIES.index("reads_lds") == 6 and nr._lib().svt_evidence_walk_capacity(7) == 0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_reads", D.BOUNDARIES)
def test_tier_boundaries(tmp_path, n_reads, entry):
    """one window with exactly N countable, kept reads: not flagged, kept_reads == N, the host reader's bytes"""
    sites, sample, nbam = W.boundary_input(tmp_path, n_reads)
    for mode in (nr.COUNT_CLASSIC, nr.COUNT_SSO):
        want, got = _compare(sites, sample, nbam, mode, None, entry)
        assert int(got[4][0]) == n_reads
        _assert_all_equal(want, got)
        assert len(got[1]) == n_reads


@pytest.mark.parametrize("entry", ENTRIES)
def test_one_read_beyond_the_deep_tier_is_flagged_with_its_true_count(tmp_path, entry):
    sites, sample, nbam = W.boundary_input(tmp_path, D.OVER)
    want, got = _compare(sites, sample, nbam, nr.COUNT_SSO, None, entry)
    assert nr.WALK_REASONS[int(got[3][0])] == "reads" and int(got[4][0]) == D.OVER == 16385
    assert int(got[0][-1]) == 0 and len(got[1]) == 0 and not got[2].any()
    assert len(want[1]) == D.OVER                         # the host reader still succeeds


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", sorted(D.REALISTIC))
def test_realistic_deep_units(tmp_path, name, entry):
    """the random BAMs of the walk's own tests at a depth that puts their one covered unit into the band the case names; both
    count modes, max_reads values that skip and that keep the unit; no unit is flagged for any reason"""
    sites, sample, nbam, (lo, hi) = D.realistic_input(tmp_path, name)
    kept_unlimited = None
    for mode, max_reads in D.MODES:
        want, got = _compare(sites, sample, nbam, mode, max_reads, entry)
        _assert_all_equal(want, got)
        if max_reads == 1000:
            assert want[2][0] == 1 and len(want[1]) == 0, "max_reads 1000 is meant to skip the unit"
        else:
            assert want[2][0] == 0 and int(want[0][1]) > 0, "every covered unit yields records"
            assert lo <= int(got[4][0]) <= hi, "the unit keeps %d reads: outside the band %d..%d this case is for" % (int(got[4][0]), lo, hi)
            kept_unlimited = int(got[4][0])
    assert kept_unlimited is not None
    assert (want[1]["seq_l"] | want[1]["clip_l"] | want[1]["seq_r"] | want[1]["clip_r"]).any()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", ["prefixes", "behind_the_key", "one_name", "name_cap"])
def test_adversarial_names(tmp_path, case, entry):
    sites, sample, nbam = D.adversarial_input(tmp_path, case)
    records = D.adversarial_cases()[case]
    if case in D.EQUAL_KEY_NAMES:                         # the case is there for whole-name compares between equal keys: it has them
        tied = D.names_behind_equal_keys(records)
        print("%s: %d different names share their 8-byte key with another name" % (case, tied))
        assert tied == D.EQUAL_KEY_NAMES[case] == len({r["name"] for r in records})
    for mode in (nr.COUNT_CLASSIC, nr.COUNT_SSO):
        want, got = _compare(sites, sample, nbam, mode, None, entry)
        assert D.LDS < int(got[4][0]) <= D.DEEP
        if case in D.EQUAL_KEY_NAMES:
            assert int(got[4][0]) == len(records)         # (every record is kept: the key computed above is the unit's)
        _assert_all_equal(want, got)
        assert len(want[1]) > 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_mixed_call_flags_only_the_over_deep_units(tmp_path, entry):
    sites, sample, nbam = D.mixed_input(tmp_path)
    want, got = _compare(sites, sample, nbam, nr.COUNT_CLASSIC, None, entry)
    shallow, deep, over = D.tiers(got[4])
    assert len(over) == 2 and len(deep) >= 2 and any(got[4][u] > 0 for u in shallow), (shallow, deep, over)
    assert max(int(got[4][u]) for u in deep) > 8192
    assert np.flatnonzero(got[3]).tolist() == over and all(nr.WALK_REASONS[int(got[3][u])] == "reads" for u in over)
    D.assert_units_equal(want, got[0], got[1], got[2], shallow + deep)
    for u in over:
        assert got[0][u + 1] == got[0][u] and want[0][u + 1] > want[0][u]


def test_abi_of_the_deep_additions(tmp_path):
    """the C view of svt_evidence_deep_stats and SVT_WALK_CAP_READS_LDS against the ctypes binding; the ABI version stays 19"""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svtyper_reads.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(svt_evidence_deep_stats), '
                   'offsetof(svt_evidence_deep_stats, units_deep), offsetof(svt_evidence_deep_stats, reads_deep), '
                   'offsetof(svt_evidence_deep_stats, workspace_bytes), offsetof(svt_evidence_deep_stats, deep_walk_s), '
                   'SVT_WALK_CAP_READS_LDS, SVT_WALK_CAP_READS, SVT_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, o0, o1, o2, o3, cap_lds, cap_reads, abi = (int(x) for x in subprocess.check_output([str(exe)]).split())
    S = nr._DeepStats
    assert (size, o0, o1, o2, o3) == (C.sizeof(S), S.units_deep.offset, S.reads_deep.offset, S.workspace_bytes.offset, S.deep_walk_s.offset)
    assert size == 32 and (cap_lds, cap_reads) == (6, 0)
    assert abi == hip.ABI_VERSION == 19
    L = nr._lib()
    assert hasattr(L, "svt_evidence_device_deep_stats")
    assert (L.svt_evidence_walk_capacity(cap_reads), L.svt_evidence_walk_capacity(cap_lds)) == (16384, 1024)
    fresh = []                                            # the figures are per thread: a thread that made no device call has zeros
    t = threading.Thread(target=lambda: fresh.append(nr.deep_stats()))
    t.start()
    t.join()
    assert fresh == [{"units_deep": 0, "reads_deep": 0, "workspace_bytes": 0, "deep_walk_s": 0.0}]
    with pytest.raises(hip.SvtyperHipError):
        hip._check(L.svt_evidence_device_deep_stats(None))


def test_deep_walk_under_asan_and_ubsan(asan_env):
    """the host build of the deep tier under AddressSanitizer + UndefinedBehaviorSanitizer (host code only), once over a
    realistic deep input with tied names, a boundary and the long run of one name"""
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider", "tests/test_deep_units_host.py",
                        "-k", "(test_realistic_deep_units and high_tied) or (test_tier_boundaries and 16384) or (test_adversarial_names and one_name)"],
                       cwd=ROOT, env=asan_env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""The one-source evidence walk (svtyper_amd/csrc/svt_evidence_walk.h) under AddressSanitizer + UndefinedBehaviorSanitizer: the
host build of the header inside `make -C svtyper_amd/csrc asan` (svt_reads.cpp instantiates it for svt_bam_evidence_walk_host).
Its CPU tests and the corrupted-BAM corpus of tools/fuzz_bam.py --walk run against that library in a subprocess with the
sanitizer runtime preloaded, as tests/test_sanitizers.py drives the other host code.  Host code only: no device is involved."""
import os
import subprocess
import sys

import pytest

from test_sanitizers import ROOT, asan_env  # noqa: F401  (the module-scoped fixture that builds the instrumented library)


def test_walk_tests_under_asan_and_ubsan(asan_env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        "tests/test_evidence_walk_host.py"], cwd=ROOT, env=asan_env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_corrupted_bams_through_the_walk_under_asan_and_ubsan(asan_env):
    env = dict(asan_env, SVT_FUZZ_ITERS="24", SVT_FUZZ_WALK="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_bam.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "crash" not in r.stdout and ("ok" in r.stdout or "error" in r.stdout), r.stdout[-1000:]

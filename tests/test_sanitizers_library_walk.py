"""The one-source library walk (svtyper_amd/csrc/svt_library_walk.h) under AddressSanitizer + UndefinedBehaviorSanitizer: the host
build of the header inside `make -C svtyper_amd/csrc asan` (svt_reads.cpp instantiates it for svt_bam_scan_libraries_walk_host).
Its CPU tests -- the fixture, the synthetic files, the envelope with its corrupted member -- run against that library in a
subprocess with the sanitizer runtime preloaded, as tests/test_sanitizers_walk.py drives the evidence walk.  Host code only."""
import subprocess
import sys

from test_sanitizers import ROOT, asan_env  # noqa: F401  (the module-scoped fixture that builds the instrumented library)


def test_library_walk_tests_under_asan_and_ubsan(asan_env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        "tests/test_library_walk_host.py"], cwd=ROOT, env=asan_env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

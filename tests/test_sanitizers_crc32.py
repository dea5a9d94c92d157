"""The one-source CRC (svtyper_amd/csrc/svt_crc32.h) and the verify paths of the host reader under AddressSanitizer +
UndefinedBehaviorSanitizer: the host build of `make -C svtyper_amd/csrc asan`.  The CPU tests of tests/test_crc32_host.py run
against that library in a subprocess with the sanitizer runtime preloaded.  Host code only: no device is involved."""
import subprocess
import sys

from test_sanitizers import ROOT, asan_env  # noqa: F401  (the module-scoped fixture that builds the instrumented library)


def test_crc32_and_verify_tests_under_asan_and_ubsan(asan_env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider", "tests/test_crc32_host.py"],
                       cwd=ROOT, env=asan_env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""The one-source DEFLATE decoder (svtyper_amd/csrc/svt_inflate.h) and the open-range arena under AddressSanitizer +
UndefinedBehaviorSanitizer: the host build of `make -C svtyper_amd/csrc asan`.  The decoder's CPU tests (clean members, the
corruption corpus and the token corpus), the open-range walk's tests and the payload-corrupting mode of tools/fuzz_bam.py run against that library in
a subprocess with the sanitizer runtime preloaded.  Host code only: no device is involved."""
import os
import subprocess
import sys

from test_sanitizers import ROOT, asan_env  # noqa: F401  (the module-scoped fixture that builds the instrumented library)


def test_inflate_and_open_walk_tests_under_asan_and_ubsan(asan_env):
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider",
                        "tests/test_inflate_host.py", "tests/test_inflate_tokens_host.py", "tests/test_walk_open_host.py"], cwd=ROOT, env=asan_env, capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert " passed" in r.stdout and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_corrupted_payloads_under_asan_and_ubsan(asan_env):
    env = dict(asan_env, SVT_FUZZ_ITERS="24", SVT_FUZZ_INFLATE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fuzz_bam.py")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-2000:])
    assert "crash" not in r.stdout and ("ok" in r.stdout or "error" in r.stdout), r.stdout[-1000:]

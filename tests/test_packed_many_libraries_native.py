"""The encoder of packed evidence for more than 256 libraries under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program: tests/native/asan_pack_many_main.cpp (its own main, svt_pack.cpp compiled into it with
-fsanitize=address,undefined -- the scheme of the ThreadSanitizer harness tests/native/tsan_pack_main.cpp) packs batches of
300 and 4 200 libraries and one that alternates across the short / wide switch boundary through every form of the encoder,
compares their bytes, and asks for the answers that stay (slot array too small, library index beyond the batch, no flag).
Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


def test_many_libraries_encoder_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_pack_many")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_pack_many_main.cpp"),
           os.path.join(CSRC, "svt_pack.cpp"), "-o", exe, "-lpthread"]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    batches = [l for l in lines if " wide switches" in l]
    assert len(batches) == 4, lines
    for l in batches:                                    # every batch held both forms of the switch
        n_short, n_wide = int(l.split(" short and ")[0].split()[-1]), int(l.split(" short and ")[1].split()[0])
        assert n_short > 0 and n_wide > 0, l

"""The first-occurrence rule (svtyper_amd/csrc/svt_bam_first_rules.h: the bounds-checked key, key_equal, key_hash and the host
twin of the pass) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
tests/native/asan_bam_first_main.cpp (its own main, the header compiled into it with -fsanitize=address,undefined).  The corpus
of tests/bamfirstcases.py, the malformed records included, as a stream in a heap buffer of exactly its length and again with
every record in a buffer that ends at its last byte -- so a read past a record's span is caught, not only one past the stream.
Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import bamfirstcases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


def cases_text(corpus):
    rows = []
    for name in sorted(corpus):
        spans = corpus[name]
        keep, bad = F.restate(spans)
        want = "!%d" % bad if bad else ",".join(str(k) for k in keep) or "-"
        rows.append("C %s %s" % (",".join(s.hex() or "." for s in spans) or "-", want))
    return "\n".join(rows) + "\n"


def test_bam_first_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_bam_first")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_bam_first_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    corpus = F.reach()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write(cases_text(corpus))
    run = subprocess.run([exe, path], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    counts = [int(part.split()[0]) for part in lines[-2].split(", ")]
    n_bad = sum(1 for spans in corpus.values() if F.restate(spans)[1])
    assert counts == [len(corpus), sum(len(s) for s in corpus.values()), n_bad] and n_bad >= 14 and len(corpus) >= 25

"""The BCF record rule, the dictionaries and the host twin (svtyper_amd/csrc/svt_bcf.h) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_bcf_main.cpp (its own main, the header compiled into it
with -fsanitize=address,undefined).  The corpus of tests/bcfcases.py as whole texts against the stream the yardstick accepted
(tests/test_bcf_host.py), each refusal, and every truncated prefix of every corpus line and of every refused line -- each in a
heap buffer that ends at the prefix, each record in a buffer of exactly its measured size.  Host code only; nothing is preloaded
and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import bcfcases as X
import bcfreader as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"columns": 1, "contig": 2, "pos": 3, "filter": 4, "info_key": 5, "format_key": 6, "info_value": 7, "format_value": 8, "samples": 9, "qual": 10}


def cases_text():
    from svtyper_amd import native_reads as nr
    rows = ["H %s" % X.header().encode().hex()]
    text = X.corpus_text()
    for flags in (0, 1, 2, 3):
        made = nr.bcf_encode(text.encode(), sort=bool(flags & 1))
        _head, d, records, _ = R.read_bcf(made["bytes"].tobytes())            # (what goes in as expected is what the yardstick reads)
        assert len(records) == len(X.LINES)
        rows.append("T %s %d %s" % (text.encode().hex(), flags, made["bytes"].tobytes().hex()))
    number = X.header().count("\n") + 2
    for _name, line, kind, _key in X.REFUSALS:
        bad = X.header() + X.LINES[1][1] + "\n" + line + "\n" + X.LINES[2][1] + "\n"
        rows.append("T %s 0 !%d,%d" % (bad.encode().hex(), number, KINDS[kind]))
    prefixes = [line for _name, line in X.LINES] + [r[1] for r in X.REFUSALS]
    rows += ["P %s" % ((line + "\n").encode().hex()) for line in prefixes]
    return "\n".join(rows) + "\n", 4 + len(X.REFUSALS), sum(len(p.encode()) + 2 for p in prefixes)


def test_bcf_rule_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_bcf")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_bcf_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_prefixes = cases_text()
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    got_cases, _got_records, got_prefixes = (int(part.split()[0]) for part in lines[-2].split(", "))
    assert got_cases == n_cases and got_prefixes == n_prefixes and n_prefixes > 30000

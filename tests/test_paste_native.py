"""The per-line rule of the paste, the host twin of its kernels, the slow path and the builder of a line's first columns
(svtyper_amd/csrc/svt_vcf_paste.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
tests/native/asan_vcf_paste_main.cpp (its own main, the header compiled into it with -fsanitize=address,undefined).  The body of
every case of tests/pastecases.py as one block against the golden bytes or the expected refusal, and every truncated prefix of
the distinct lines of the small cases -- each text in a heap buffer of exactly its length, each output in a buffer of exactly
its size.  Host code only; nothing is preloaded and no Python-loaded code is involved."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import pastecases as P

from svtyper_amd import native_reads as nr
from svtyper_amd import paste

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"ValueError": (nr.PASTE_BAD_QUAL,), "IndexError": (nr.PASTE_BAD_ALLELE, nr.PASTE_BAD_COLUMNS)}


def body_of(text):
    lines = text.splitlines(True)
    at = next(k for k, l in enumerate(lines) if not l.startswith("##"))
    return [l.rstrip("\n") for l in lines[:at]], lines[at], lines[at + 1:]


def cases_text():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "paste_cases.json.gz"), "rt") as f:
        golden = json.load(f)
    expected = {c["name"]: c["expected"] for c in golden["cases"]}
    rows, prefixes, n_cases, slow = [], {}, 0, 0
    for case in P.cases():
        header, chrom, master = body_of(case["master"] if case["master"] is not None else case["inputs"][0])
        inputs = [body_of(t)[2] for t in case["inputs"]]
        flags = (nr.PASTE_SUM_QUALS if case["sum_quals"] else 0) | (nr.PASTE_AFREQ if case["afreq"] else 0)
        table = paste.afreq_header(header, chrom, golden["file_date"], False)[1] if case["afreq"] else b""
        n = min(len(master), min(len(i) for i in inputs))           # (a short input: the lines in front of its end)
        text = "".join("".join(f[:n]) for f in [master] + inputs).encode()
        want = expected[case["name"]]
        if want["status"] == 0 or case["error"]["message"]:
            made = "".join(want["stdout"].splitlines(True)[-n:]).encode().hex() if want["status"] == 0 else None
            if made is None:                        # the short input's case: its first lines are like any others
                made = nr.vcf_paste(text, [k * n for k in range(len(inputs) + 1)], len(inputs), n, flags, table)[0].hex()
            slow += case["slow_lines"]
        else:
            kinds = KINDS[want["exception"]]
            line = case["error"]["line"] - (len(header) + 1 if case["error"]["file"] == 0 else 2)
            made = "!%d,%d,%d" % (line, case["error"]["file"], kinds[0])
        rows.append("C %d %d %d %s %s %s" % (flags, len(inputs), n, table.hex() or "-", text.hex(), made))
        n_cases += 1
        if len(inputs) <= 3:
            for f in [master] + inputs:
                for line in f[:12]:
                    prefixes.setdefault((flags, table, line.rstrip("\n")), None)
    rows += ["P %d %s %s" % (flags, table.hex() or "-", line.encode().hex()) for flags, table, line in prefixes]
    return "\n".join(rows) + "\n", n_cases, sum(len(line.encode()) + 1 for _f, _t, line in prefixes), slow


def test_paste_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_vcf_paste")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_vcf_paste_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_prefixes, slow = cases_text()
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "cases %d prefixes %d host_lines %d" % (n_cases, n_prefixes, slow)

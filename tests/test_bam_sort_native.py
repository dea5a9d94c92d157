"""The per-record rule, the host span table, the order, the member cut and the index fold (svtyper_amd/csrc/svt_bam_sort_rules.h,
svt_bai_index.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_bam_sort_main.cpp
(its own main, the headers compiled into it with -fsanitize=address,undefined).  The corpus of tests/baicases.py against the
checker's table and order, and every truncated prefix of every corpus record (as cut, and again with a block_size that claims
the cut is whole) -- each stream in a heap buffer of exactly its length.  Host code only; nothing is preloaded and no
Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import baicases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
SHARES = 4      # runs of the program at the same time


def cases_text():
    rows, prefixes = [], []
    cases = dict(B.CASES)
    cases["single_pass"], cases["every_digit"] = B.single_pass_case(), B.every_digit_case()
    for name in sorted(cases):
        case = cases[name]
        table = "".join("%d,%d,%d,%d,%d,%d,%d;" % row for row in B.table(0, case.records, case.n_ref)) or "-"
        bad, kind = B.first_bad(case.records, case.n_ref)
        order = "!%d,%d" % (bad, kind) if bad else ",".join(str(i) for i in B.order(case.records, case.n_ref)) or "-"
        rows.append("C %d %s %s %s" % (case.n_ref, ",".join(r.hex() for r in case.records) or "-", table, order))
        prefixes += [(case.n_ref, raw) for raw in case.records]
    # every record of every case, whole; dealt to SHARES runs of the program by size, the largest first, so that they end together
    shares = [rows] + [[] for _ in range(SHARES - 1)]
    weight = [sum(len(r) for r in rows) // 64] + [0] * (SHARES - 1)
    for n_ref, raw in sorted(prefixes, key=lambda p: -len(p[1])):
        if len(raw) > 8192:                         # the long record: its cuts in SHARES ranges of equal cost, one per run
            edges = [int((len(raw) + 1) * (k / SHARES) ** 0.5) for k in range(SHARES)] + [len(raw) + 1]
            for k in range(SHARES):
                shares[k].append("P %d %s %d %d" % (n_ref, raw.hex(), edges[k], edges[k + 1]))
                weight[k] += len(raw) * len(raw) // 4096 // SHARES
            continue
        k = weight.index(min(weight))
        shares[k].append("P %d %s" % (n_ref, raw.hex()))
        weight[k] += len(raw) * len(raw) // 4096 + len(raw)     # (a prefix costs its copy, a record has as many as bytes)
    return ["\n".join(share) + "\n" for share in shares], len(cases), sum(len(raw) + 1 for _n_ref, raw in prefixes)


def test_bam_sort_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_bam_sort")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_bam_sort_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    texts, n_cases, n_prefixes = cases_text()
    runs = []
    for k, text in enumerate(texts):                # host programs side by side: the prefixes are independent of each other
        cases = str(tmp_path / ("cases%d.txt" % k))
        with open(cases, "w") as f:
            f.write(text)
        runs.append(subprocess.Popen([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                                     stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    got_cases = got_prefixes = 0
    for run in runs:
        out, err = run.communicate(timeout=600)
        assert run.returncode == 0 and "AddressSanitizer" not in err and "runtime error" not in err, (out[-2000:], err[-3000:])
        lines = out.strip().splitlines()
        assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
        counts = [int(part.split()[0]) for part in lines[-2].split(", ")]
        got_cases, got_prefixes = got_cases + counts[0], got_prefixes + counts[2]
    assert got_cases == n_cases and got_prefixes == n_prefixes and n_cases > 25 and n_prefixes > 500000

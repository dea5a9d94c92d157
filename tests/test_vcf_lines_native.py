"""The per-line rule, the host line table, the order, the gather and the index fold (svtyper_amd/csrc/svt_vcf_lines.h,
svt_tbx_index.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_vcf_lines_main.cpp
(its own main, the headers compiled into it with -fsanitize=address,undefined).  The corpus of tests/tbxcases.py against the
checker's table and sorted text, and every truncated prefix of every corpus line -- each text in a heap buffer of exactly its
length.  Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import tbxcases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


def cases_text():
    rows = []
    texts = dict(X.TABLE_TEXTS)
    texts.update(X.ORDERS)
    texts.update({"line:" + name: line for name, (line, _want) in X.LINES.items()})
    for name in sorted(texts):
        text = texts[name]
        table = "".join("%d,%d,%d,%d,%d,%d;" % row for row in X.table(text)) or "-"
        lines = X.split_lines(text)
        sortable = all(X.parse(l)[3] in (0, X.RANGE) for l in lines[X.header_count(lines):])
        if sortable and text and not text.endswith(b"\n"):
            sortable = None         # (the writer gives such a text its newline first: the bare gather is not asked for it)
        want = (X.sorted_text(text).hex() or "-") if sortable else "!"
        if sortable is None:
            continue
        rows.append("T %s %s %s" % (text.hex() or "-", table, want))
    prefixes = [line for _name, (line, _want) in sorted(X.LINES.items())] + [X.ORDERS["undeclared_contig"], X.CONTIG_HEADER]
    rows += ["P %s" % line.hex() for line in prefixes]
    return "\n".join(rows) + "\n", sum(r.startswith("T") for r in rows), sum(len(p) + 1 for p in prefixes)


def test_vcf_lines_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_vcf_lines")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_vcf_lines_main.cpp"), "-o", exe]
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
    got_cases, _got_lines, got_prefixes = (int(part.split()[0]) for part in lines[-2].split(", "))
    assert got_cases == n_cases and got_prefixes == n_prefixes and n_cases > 60

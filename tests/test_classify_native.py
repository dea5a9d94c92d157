"""The native layers of svtyper_amd.classify without a GPU: svt_classify_line against the numpy dtype, and the per-line rule, the
host twin of the kernel, the plain C++ of the marked lines and the writer (svtyper_amd/csrc/svt_vcf_classify.h) under
AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_vcf_classify_main.cpp (its own main,
the header compiled into it with -fsanitize=address,undefined).  The body of every case of tests/classifycases.py without an
annotation as one block against the golden bytes or the expected refusal, and every truncated prefix of the distinct lines of the
narrow cases (malformed lines among them) -- each text in a heap buffer of exactly its length.  Host code only; nothing is
preloaded and no Python-loaded code is involved."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import classifycases as K
import test_classify_host as H

from svtyper_amd import native_reads as nr
from svtyper_amd import cohort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"ValueError": (nr.CLASSIFY_BAD_POS, nr.CLASSIFY_BAD_QUAL, nr.CLASSIFY_BAD_NUMBER), "KeyError": (nr.CLASSIFY_BAD_KEY, nr.CLASSIFY_BAD_GENDER),
         "IndexError": (nr.CLASSIFY_BAD_COLUMNS,), None: (nr.CLASSIFY_BAD_FORMAT,)}


def test_structure_matches_the_header():
    """include/svtyper_reads.h: svt_classify_line, field by field"""
    with open(os.path.join(ROOT, "include", "svtyper_reads.h")) as f:
        body = re.search(r"typedef struct svt_classify_line \{(.*?)\} svt_classify_line;", f.read(), re.S).group(1)
    fields, at = [], 0
    for kind, names in re.findall(r"(double|uint32_t) ([^;]+);", body):
        for name in names.split(","):
            size = 8 if kind == "double" else 4
            fields.append((name.strip(), at, size))
            at += size
    assert at == nr.CLASSIFY_LINE.itemsize == 64
    assert fields == [(name, nr.CLASSIFY_LINE.fields[name][1], nr.CLASSIFY_LINE.fields[name][0].itemsize) for name in nr.CLASSIFY_LINE.names]
    assert all(nr.CLASSIFY_LINE.fields[name][0] == (np.float64 if size == 8 else np.uint32) for name, _at, size in fields)


def tables_of(case):
    lines = case["vcf"].splitlines(True)
    header = [l for l in lines[:next((k for k, l in enumerate(lines) if not l.startswith("#")), len(lines))]]
    _ff, _ref, _filters, infos, _alts, formats = cohort.header_attributes([h.rstrip("\n") for h in header if h.startswith("##")], ValueError)
    samples = next((h.rstrip().split("\t")[9:] for h in header if not h.startswith("##")), [])
    genders = dict(l.split("\t") for l in case["gender"].splitlines())
    excluded = set((case["exclude"] or "").splitlines())
    code = lambda s, g: 1 if genders.get(s) == g else nr.CLASSIFY_NO_GENDER if s not in genders else 0
    row = [len(samples), bytes(code(s, "1") for s in samples), bytes(code(s, "2") for s in samples), bytes(s in excluded for s in samples),
           cohort.format_table(formats), cohort.info_table(infos)]
    return " ".join(str(v) if isinstance(v, int) else (v.hex() or "-") for v in row), "".join(lines[len(header):]), len(header)


def cases_text():
    rows, prefixes, n_cases, slow = [], {}, 0, 0
    for case in K.cases():
        if case["annotation"] is not None or not case["vcf"].endswith("\n"):
            continue
        tables, body, n_header = tables_of(case)
        if not body:
            continue
        want = H.EXPECTED[case["name"]]["expected"]
        if want["status"] == 0:
            written = want["stdout"].splitlines(True)
            made = "".join(written[next(k for k, l in enumerate(written) if l.startswith("#CHROM")) + 1:]).encode().hex() or "-"
            slow += case["slow_lines"]
        else:
            kind = getattr(nr, "CLASSIFY_BAD_" + case["kind"])       # what the corpus says of the case, not what the code gives
            assert kind in KINDS[want["exception"]], case["name"]
            made = "!%d,%d" % (case["error"] - n_header, kind)
        o = case["options"]
        rows.append("C %s %r %r %s %s" % (tables, o["slope_threshold"], o["rsquared_threshold"], body.encode().hex(), made))
        n_cases += 1
        if case["n_samples"] <= 10:
            for line in body.splitlines()[:4]:
                prefixes.setdefault((tables, line), None)
    rows += ["P %s %s" % (tables, line.encode().hex()) for tables, line in prefixes]
    return "\n".join(rows) + "\n", n_cases, sum(len(line.encode()) + 1 for _t, line in prefixes), slow


def test_classify_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_vcf_classify")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_vcf_classify_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_prefixes, slow = cases_text()
    assert n_cases > 70 and n_prefixes > 10000
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "cases %d prefixes %d host_lines %d" % (n_cases, n_prefixes, slow)

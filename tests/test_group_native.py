"""The native layers of svtyper_amd.group_multiline without a GPU: svt_group_line and svt_group_out against their numpy dtypes, the
entry points' host side through ctypes, and the per-line rule, the host twin of the scan kernel, the plain C++ of the marked
lines, the join and the writer (svtyper_amd/csrc/svt_vcf_group.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program: tests/native/asan_vcf_group_main.cpp (its own main, the header compiled into it with
-fsanitize=address,undefined).  The body of every case of tests/groupcases.py against the golden bytes and the expected refusal,
and every truncated prefix of the distinct lines of the narrow cases (malformed lines among them) -- each text in a heap buffer of
exactly its length.  Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import groupcases as K
import test_group_host as H

from svtyper_amd import cohort, group_multiline, hip
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"ValueError": (nr.GROUP_BAD_POS, nr.GROUP_BAD_QUAL, nr.GROUP_BAD_NUMBER), "KeyError": (nr.GROUP_BAD_KEY,),
         "IndexError": (nr.GROUP_BAD_COLUMNS, nr.GROUP_BAD_ALT), "AttributeError": (nr.GROUP_BAD_BARE,),
         None: (nr.GROUP_BAD_FORMAT, nr.GROUP_BAD_EIGHT)}


def test_structures_match_the_header():
    """include/svtyper_reads.h: svt_group_line and svt_group_out, field by field, and the constants beside them"""
    with open(os.path.join(ROOT, "include", "svtyper_reads.h")) as f:
        header = f.read()
    kinds = {"uint64_t": (8, np.uint64), "uint32_t": (4, np.uint32)}
    for name, dtype, size in (("svt_group_line", nr.GROUP_LINE, 40), ("svt_group_out", nr.GROUP_OUT, 8)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        fields, at = [], 0
        for kind, names in re.findall(r"(uint64_t|uint32_t) ([^;]+);", body):
            for field in names.split(","):
                fields.append((field.strip(), at, kinds[kind][1]))
                at += kinds[kind][0]
        assert at == dtype.itemsize == size
        assert fields == [(field, dtype.fields[field][1], dtype.fields[field][0].type) for field in dtype.names]
    for name, value in re.findall(r"#define SVT_(GROUP_(?:BND|HAS_MATE|CI|SLOW\w*|BAD_\w+)) (\d+)u", header):
        assert getattr(nr, name) == int(value), name
    keys = re.findall(r"#define SVT_GROUP_KEY_(\w+) (\d+)u", header)
    assert tuple(k for k, _v in sorted(keys, key=lambda kv: int(kv[1]))) == nr.GROUP_KEYS


def tables_of(case):
    lines = case["vcf"].splitlines(True)
    n_header = next((k for k, l in enumerate(lines) if not l.startswith("#")), len(lines))
    _ff, _ref, infos, _alts, formats, samples = group_multiline.header_tables(lines[:n_header])
    body = "".join(lines[n_header:])
    if body and not body.endswith("\n"):
        body += "\n"                                                # (as the module hands it over)
    return len(samples), cohort.format_table(formats), cohort.info_table(infos), body, n_header


def test_entry_points_through_ctypes():
    """svt_vcf_group_host, _write and _take as the module calls them; what they refuse"""
    case = next(c for c in H.CASES if c["name"] == "format_out_of_order_on_the_first")
    n, formats, infos, body, _h = tables_of(case)
    lines, plan, report = nr.vcf_group(body.encode(), n, formats)
    assert report["host_lines"] == 1 and report["bad_line"] == 0 and report["host_join"] == 1
    assert list(lines["slow"]) == [nr.GROUP_SLOW_FORMAT, 0] and lines["flags"][1] == nr.GROUP_BND | nr.GROUP_HAS_MATE | nr.GROUP_CI
    assert list(lines["off"]) == [0, len(body.splitlines(True)[0])] and plan.tolist() == [(0, 0), (1, 0)]
    out, out_off, written = nr.vcf_group_write(body.encode(), n, infos, formats, lines, plan)
    golden = H.EXPECTED[case["name"]]["expected"]["stdout"]
    assert out.decode() == golden[golden.index("\n1\t") + 1:] and written["bad_line"] == 0
    assert out_off[0] == 0 and out_off[-1] == len(out) and out[int(out_off[1]) - 1:int(out_off[1])] == b"\n"
    both = np.array([(1, 1), (0, 1), (0, 0)], nr.GROUP_OUT)         # any plan over the lines is written as it stands
    out, out_off, written = nr.vcf_group_write(body.encode(), n, infos, formats, lines, both)
    assert len(out.splitlines()) == 3 and written["bad_line"] == 0
    with pytest.raises(hip.SvtyperHipError):                        # an entry that names no line
        nr.vcf_group_write(body.encode(), n, infos, formats, lines, np.array([(2, 0)], nr.GROUP_OUT))
    outside = lines.copy()
    outside["len"][1] += 2
    with pytest.raises(hip.SvtyperHipError):                        # a record that runs past the text
        nr.vcf_group_write(body.encode(), n, infos, formats, outside, plan)
    with pytest.raises(hip.SvtyperHipError):                        # GT is not the first FORMAT id
        nr.vcf_group(body.encode(), n, b"SQ\nGT\n")
    empty, nothing, report = nr.vcf_group(b"", n, formats)
    assert len(empty) == 0 and len(nothing) == 0 and report["host_lines"] == 0
    if hip.device_count() < 1:                                      # (no GPU: the device's entry says so, it does not fall back)
        with pytest.raises(hip.SvtyperHipError):
            nr.vcf_group(body.encode(), n, formats, device=0)
    else:
        with pytest.raises(hip.SvtyperHipError):
            nr.vcf_group(body.encode(), n, formats, device=0, hash_bits=65)


def cases_text():
    rows, prefixes, n_cases, slow = [], {}, 0, 0
    for case in K.cases():
        if case["kind"] is None and case["error"] is not None:      # (Python's: no #CHROM line)
            continue
        n, formats, infos, body, n_header = tables_of(case)
        if not body:
            continue
        tables = "%d %s %s" % (n, formats.hex(), infos.hex())
        want = H.EXPECTED[case["name"]]["expected"]
        written = want["stdout"].splitlines(True)
        made = "".join(written[next(k for k, l in enumerate(written) if l.startswith("#CHROM")) + 1:]).encode().hex() or "-"
        slow += case["slow_lines"]
        death = "-"
        if want["status"]:
            kind = getattr(nr, "GROUP_BAD_" + case["kind"])         # what the corpus says of the case, not what the code gives
            assert kind in KINDS[want["exception"]], case["name"]
            death = "!%d,%d" % (case["error"] - n_header, kind)
        rows.append("C %s %s %s %s" % (tables, body.encode().hex(), made, death))
        n_cases += 1
        if not case["name"].startswith("pairs_"):
            for line in body.splitlines()[:4]:
                prefixes.setdefault((tables, line), None)
    rows += ["P %s %s" % (tables, line.encode().hex()) for tables, line in prefixes]
    return "\n".join(rows) + "\n", n_cases, sum(len(line.encode()) + 1 for _t, line in prefixes), slow


def test_group_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_vcf_group")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_vcf_group_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_prefixes, slow = cases_text()
    assert n_cases > 90 and n_prefixes > 10000
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "cases %d prefixes %d host_lines %d" % (n_cases, n_prefixes, slow)

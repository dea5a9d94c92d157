"""The native layers of svtyper_amd.update_info without a GPU: svt_update_info_line against the numpy dtype, the five entry points'
host side through ctypes, and the per-line rule, the host twin of the kernel, the plain C++ of the marked lines and the writer
(svtyper_amd/csrc/svt_vcf_update_info.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program:
tests/native/asan_vcf_update_info_main.cpp (its own main, the header compiled into it with -fsanitize=address,undefined).  The body
of every case of tests/updateinfocases.py as one block against the golden bytes or the expected refusal, and every truncated
prefix of the distinct lines of the narrow cases (malformed lines among them) -- each text in a heap buffer of exactly its length.
Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_update_info_host as H
import updateinfocases as K

from svtyper_amd import hip
from svtyper_amd import native_reads as nr
from svtyper_amd import cohort, update_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"ValueError": (nr.UPDATE_INFO_BAD_POS, nr.UPDATE_INFO_BAD_QUAL, nr.UPDATE_INFO_BAD_NUMBER), "KeyError": (nr.UPDATE_INFO_BAD_KEY,),
         "IndexError": (nr.UPDATE_INFO_BAD_COLUMNS,), None: (nr.UPDATE_INFO_BAD_FORMAT, nr.UPDATE_INFO_BAD_EIGHT)}


def test_structure_matches_the_header():
    """include/svtyper_reads.h: svt_update_info_line, field by field, and the constants beside it"""
    with open(os.path.join(ROOT, "include", "svtyper_reads.h")) as f:
        header = f.read()
    body = re.search(r"typedef struct svt_update_info_line \{(.*?)\} svt_update_info_line;", header, re.S).group(1)
    kinds = {"int64_t": (8, np.int64), "uint64_t": (8, np.uint64), "uint32_t": (4, np.uint32)}
    fields, at = [], 0
    for kind, names in re.findall(r"(int64_t|uint64_t|uint32_t) ([^;]+);", body):
        for name in names.split(","):
            fields.append((name.strip(), at, kinds[kind][1]))
            at += kinds[kind][0]
    assert at == nr.UPDATE_INFO_LINE.itemsize == 40
    assert fields == [(name, nr.UPDATE_INFO_LINE.fields[name][1], nr.UPDATE_INFO_LINE.fields[name][0].type) for name in nr.UPDATE_INFO_LINE.names]
    for name, value in re.findall(r"#define SVT_(UPDATE_INFO_\w+) (\d+)u", header):
        assert getattr(nr, name) == int(value), name


def tables_of(case):
    lines = case["vcf"].splitlines(True)
    n_header = next((k for k, l in enumerate(lines) if not l.startswith("#")), len(lines))
    _ff, _ref, infos, _alts, formats, samples = update_info.header_tables(lines[:n_header])
    return len(samples), cohort.format_table(formats), cohort.info_table(infos), "".join(lines[n_header:]), n_header


def test_entry_points_through_ctypes():
    """svt_vcf_update_info_host, _write and _take as the module calls them, on one block of two lines; what they refuse"""
    case = next(c for c in H.CASES if c["name"] == "format_out_of_header_order")
    n, formats, infos, body, _h = tables_of(case)
    records, info = nr.vcf_update_info(body.encode(), n, formats)
    assert info["host_lines"] == 1 and info["bad_line"] == 0 and list(records["route"]) == [nr.UPDATE_INFO_PLAIN, nr.UPDATE_INFO_RULE]
    assert list(records["flags"]) == [nr.UPDATE_INFO_SLOW_FORMAT, 0] and (records["num_pos"] == n).all()
    columns = [c.split(":") for c in body.splitlines()[1].split("\t")[9:]]
    assert records["pe"][1] == sum(int(c[5]) for c in columns) and records["sr"][1] == sum(int(c[4]) for c in columns)
    assert np.array([records["sum_sq"][1]], np.uint64).view(np.float64)[0] == sum((float(c[2]) for c in columns), 0.0)
    out, out_off, written = nr.vcf_update_info_write(body.encode(), n, infos, formats, records)
    golden = H.EXPECTED[case["name"]]["expected"]["stdout"]
    assert out.decode() == golden[golden.index("\n1\t") + 1:] and written["bad_line"] == 0
    assert out_off[0] == 0 and out_off[-1] == len(out) and out[int(out_off[1]) - 1:int(out_off[1])] == b"\n"
    with pytest.raises(hip.SvtyperHipError):                        # a record too few
        nr.vcf_update_info_write(body.encode(), n, infos, formats, records[:1])
    with pytest.raises(hip.SvtyperHipError):                        # GT is not the first FORMAT id
        nr.vcf_update_info(body.encode(), n, b"SQ\nGT\n")
    empty, info = nr.vcf_update_info(b"", n, formats)
    assert len(empty) == 0 and info["host_lines"] == 0
    if hip.device_count() < 1:                                      # (no GPU: the device's entry says so, it does not fall back)
        with pytest.raises(hip.SvtyperHipError):
            nr.vcf_update_info(body.encode(), n, formats, device=0)


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
        if want["status"] == 0:
            written = want["stdout"].splitlines(True)
            made = "".join(written[next(k for k, l in enumerate(written) if l.startswith("#CHROM")) + 1:]).encode().hex() or "-"
            slow += case["slow_lines"]
        else:
            kind = getattr(nr, "UPDATE_INFO_BAD_" + case["kind"])    # what the corpus says of the case, not what the code gives
            assert kind in KINDS[want["exception"]], case["name"]
            made = "!%d,%d" % (case["error"] - n_header, kind)
        rows.append("C %s %s %s" % (tables, body.encode().hex(), made))
        n_cases += 1
        if case["n_samples"] <= 10:
            for line in body.splitlines()[:4]:
                prefixes.setdefault((tables, line), None)
    rows += ["P %s %s" % (tables, line.encode().hex()) for tables, line in prefixes]
    return "\n".join(rows) + "\n", n_cases, sum(len(line.encode()) + 1 for _t, line in prefixes), slow


def test_update_info_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_vcf_update_info")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_vcf_update_info_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_prefixes, slow = cases_text()
    assert n_cases > 50 and n_prefixes > 10000
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.strip().splitlines()[-1] == "cases %d prefixes %d host_lines %d" % (n_cases, n_prefixes, slow)

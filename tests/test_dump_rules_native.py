"""The dump rules (svtyper_amd/csrc/svt_dump_rules.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
program: tests/native/asan_dump_rules_main.cpp (its own main, the header compiled into it with -fsanitize=address,undefined).
Every record of the edge corpus (tests/dumpcases.py), and records with the tag areas the corpus cannot have -- shorter than an RG,
cut, malformed --, in each of the three tag states, against what bam.AlignmentFile.write emits for the read in that state; every
truncated prefix has to come back as outside the envelope.  Host code only; nothing is preloaded and no Python-loaded code is
involved."""
import os
import shutil
import subprocess
import types

import pytest

import bamwriter as bw
import dumpcases as D
from svtyper_amd import bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")

# tag areas without RG: nothing, one field of every size, an XV alone and XV beside others -- and areas the rules have to refuse:
# bytes behind the last field, an unknown type, a Z without its NUL, a B array beyond the record
SHORT_AREAS = [[], [("XV", "A", "R")], [("XV", "c", -1)], [("XV", "s", 2)], [("XV", "Z", "R")], [("XV", "Z", "")], [("NM", "i", 5)],
               [("XV", "i", 5)], [("XV", "f", 1.5)], [("XV", "H", "1AE3")], [("XV", "B", ("C", []))], [("XV", "B", ("i", [1, 2]))],
               [("NM", "C", 1), ("XV", "Z", "AB")], [("XV", "A", "A"), ("XV", "A", "R"), ("XV", "Z", "x")]]
REFUSED_AREAS = [b"X", b"XV", b"XVA", b"NMC\x01X", b"NMC\x01XVAR\0\0", b"XVQx", b"XVZabc", b"XVBc\x05\0\0\0\1\2", b"XVBq\0\0\0\0",
                 b"XVi\1\2\3"]


def written(body, state):
    """what bam.AlignmentFile.write emits for the record `body` (behind block_size) with XV set to R (1), to A (2) or not at all"""
    seg = bam.AlignedSegment(None, body)
    if state:
        seg.set_tag("XV", "RA"[state - 1])
    seg.query_sequence = None
    got = []
    stub = types.SimpleNamespace(_writer=types.SimpleNamespace(write_record=got.append), filename="stub")
    bam.AlignmentFile.write(stub, seg)
    return got[0]


def cases_text():
    records = [bw.encode_record(r)[0] for r in D.records(long_name=True)]
    base = D.records()[0]
    records += [bw.encode_record(dict(base, name="s%d" % k, tags=tags))[0] for k, tags in enumerate(SHORT_AREAS)]
    lines = ["E %d %s %s" % (state, rec.hex(), written(rec[4:], state).hex()) for rec in records for state in (0, 1, 2)]
    refused = [bw.encode_record(dict(base, name="r%d" % k, tags=[("", "raw", area)]))[0] for k, area in enumerate(REFUSED_AREAS)]
    lines += ["E %d %s -" % (state, rec.hex()) for rec in refused for state in (1, 2)]
    return "\n".join(lines) + "\n", len(records), len(refused)


def test_dump_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_dump_rules")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_dump_rules_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_records, n_refused = cases_text()
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    n_cases, n_outside, n_prefixes, n_emits = (int(part.split()[0]) for part in lines[-2].split(", "))
    assert n_cases == 3 * n_records + 2 * n_refused and n_outside == 2 * n_refused
    assert n_emits == 16 * 3 * n_records and n_prefixes > 50 * n_records      # (four source x four destination alignments)

"""The BCF-to-text record rule, the dictionaries by index and the host twin (svtyper_amd/csrc/svt_bcf_text.h) under AddressSanitizer
+ UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_bcf_text_main.cpp (its own main, the header compiled into
it with -fsanitize=address,undefined).  The corpus of tests/bcfcases.py as whole streams against the text the yardstick prints
(tests/bcftext.py over tests/bcfreader.py), in one chunk and in chunks of one record, by snprintf and by the exact float rule; the
hand-built streams of tests/bcftextcases.py (IDX=, the float edges) and each of its refusals; every truncation of the corpus
stream's last record; then every record of the corpus cut at every byte -- as it is, and with its two lengths set to what is left --
and changed at every byte to six other values, each in a heap buffer that ends where the record ends, each line in a buffer of
exactly its measured size.  Host code only; nothing is preloaded and no Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import bcfcases as X
import bcfreader as R
import bcftext as T
import bcftextcases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
KINDS = {"truncated": 1, "index": 2, "samples": 3, "type": 4, "count": 5, "gt": 6, "length": 7}


def sweep_walks(stream):
    """the walks an M row makes over `stream`: per record of z bytes the record itself, z prefixes, z - 8 prefixes with their lengths
    set again, and six values at every byte (every seventh above 4096 bytes), each by snprintf and by the exact rule"""
    starts = R.read_bcf(stream)[3]
    sizes = [b - a for a, b in zip(starts, starts[1:] + [len(stream)])]
    return sum(2 * (1 + z + max(z - 8, 0) + 6 * len(range(0, z, 7 if z > 4096 else 1))) for z in sizes)


def cases_text():
    from svtyper_amd import native_reads as nr
    rows = []
    corpus = nr.bcf_encode(X.corpus_text().encode())["bytes"].tobytes()
    want, _d, records = T.text(corpus, R)
    assert len(records) == len(X.LINES)
    for flags in (0, 2):
        for block in (1 << 40, 1):
            rows.append("S %s %d %d %s" % (corpus.hex(), flags, block, want.encode().hex()))
    idx, idx_want = C.idx_stream()
    rows.append("S %s 0 64 %s" % (idx.hex(), idx_want.encode().hex()))
    bits = C.edge_floats()
    floats = C.float_stream(bits)
    float_want = C.FLOAT_HEADER + "".join("c\t%d\t.\tN\t.\t%s\t.\tV=%s\n" % (k + 1, T.float_text(b), T.float_text(b)) for k, b in enumerate(bits))
    rows += ["S %s %d 4096 %s" % (floats.hex(), flags, float_want.encode().hex()) for flags in (0, 2)]
    for _name, kind, bad in C.refusals():
        rows.append("S %s 0 1 !2,%d" % (C.refusal_stream(bad).hex(), KINDS[kind]))
    starts = R.read_bcf(corpus)[3]
    for cut in range(starts[-1] + 1, len(corpus)):
        rows.append("S %s 2 4096 !%d,1" % (corpus[:cut].hex(), len(starts)))
    rows.append("S %s 0 4096 %s" % (corpus[:starts[-1]].hex(), "".join(want.splitlines(True)[:-1]).encode().hex()))
    n_streams = len(rows)
    shaped = nr.bcf_encode(X.shaped_text(2, 65).encode())["bytes"].tobytes()
    rows += ["M %s" % corpus.hex(), "M %s" % shaped.hex()]
    return "\n".join(rows) + "\n", n_streams + 2, sweep_walks(corpus) + sweep_walks(shaped)


def test_bcf_text_rule_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_bcf_text")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_bcf_text_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    text, n_cases, n_walks = cases_text()
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write(text)
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    got_cases, got_walks, got_lines = (int(part.split()[0]) for part in lines[-2].split(", "))
    assert got_cases == n_cases and got_walks == n_walks and n_walks > 500000 and got_lines > 10000

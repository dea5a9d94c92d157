"""The rANS 4x8 host twin and the CRAM slice decoder in a program of their own (tests/native/asan_cram_main.cpp: its own main, the
headers compiled into it with -fsanitize=address,undefined) over a corpus this test writes: the rANS corpus of tests/cramcases.py
with its malformed blocks, and the slices of CRAM files in many layouts -- intact, with every block cut short, and with bytes
changed at random.  Whatever a damaged slice decodes to, no byte outside a buffer is touched."""
import os
import random
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramcases as cc  # noqa: E402
import cramwriter as cw  # noqa: E402
from svtyper_amd import cram  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


def hx(b):
    return bytes(b).hex() or "-"


def slice_rows(tmp_path):
    rng = random.Random(11)
    rows, intact = [], 0
    for name, layout in cc.layouts():
        path = str(tmp_path / (name + ".cram"))
        cw.write_cram(path, cc.HEADER, cc.mixed_records(), layout, crai=False)
        f = cram.CramFile(path)
        at = f._first
        while True:
            c = f._container(at)
            if c is None or f._is_eof(c):
                break
            at = c.end
            for _key, comp, sl, blocks in f._slices(c):
                f._undo([comp, sl] + blocks)
                cur = cram._Cursor(sl.content)
                _ref, _start, _span, n_records = cur.itf8(), cur.itf8(), cur.itf8(), cur.itf8()

                def row(comp_b, sl_b, parts, want):
                    return "S %s %s 2 rg1,rg2 %d %d %s" % (hx(comp_b), hx(sl_b), want, len(parts),
                                                           " ".join("%d %d %s" % (b.cid, b.ctype == 5, hx(p)) for b, p in zip(blocks, parts)))
                contents = [bytes(b.content) for b in blocks]
                rows.append(row(comp.content, sl.content, contents, n_records))
                intact += 1
                for k in range(len(contents)):                   # every block cut short, one at a time
                    if contents[k]:
                        cut = list(contents)
                        cut[k] = cut[k][:len(cut[k]) // 2]
                        rows.append(row(comp.content, sl.content, cut, -1))
                for _ in range(6):                                # bytes changed at random: in a block, in a header
                    hurt = [bytearray(x) for x in contents]
                    comp_b, sl_b = bytearray(comp.content), bytearray(sl.content)
                    target = rng.choice([x for x in hurt if x] + [comp_b, comp_b, sl_b])
                    for _ in range(rng.randint(1, 3)):
                        target[rng.randrange(len(target))] = rng.randrange(256)
                    rows.append(row(comp_b, sl_b, hurt, -1))
        f.close()
    return rows, intact


def test_rans_and_slice_decoder_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_cram")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_cram_main.cpp"), "-o", exe, "-pthread"]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    rows = ["R %s %d %d %s" % (hx(block), n, -1 if status is None else status, hx(want) if want is not None and status == 0 else "-")
            for _name, block, n, want, status in cc.rans_corpus()]
    n_rans = len(rows)
    slices, intact = slice_rows(tmp_path)
    assert intact > 60 and len(slices) > 1000
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        f.write("\n".join(rows + slices) + "\n")
    r = subprocess.run([exe, cases], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[:4] == ["rans", str(n_rans), "slices", str(len(slices))] and int(last[5]) > 100

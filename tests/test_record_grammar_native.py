"""rr::walk_tags, rr::decode_core and rr::cigar_of_string (svtyper_amd/csrc/svt_record_rules.h) under AddressSanitizer +
UndefinedBehaviorSanitizer, as a stand-alone program: tests/native/asan_record_rules_main.cpp (its own main, the header compiled
into it with -fsanitize=address,undefined) walks every prefix of the grammar corpus' tag areas, of two whole records and of the
CIGAR texts, each in a heap buffer of exactly its length, with both values of stop_at_rg, and compares the answer at full
length with what grammarcases.spec_tags finds (tests/golden/record_grammar_areas.txt, which this module writes when it is run
as a program and compares with the corpus when it is run as a test).  Host code only; nothing is preloaded and no
Python-loaded code is involved."""
import os
import shutil
import subprocess

import pytest

import bamwriter as bw
import grammarcases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "record_grammar_areas.txt")
WHOLE_RECORDS = ("s08_arrays17_last", "c08")


def _area_lines(label, area):
    """the two lines of a tag area: what a walk to the end and a walk that stops behind the first RG:Z have to answer"""
    tags = list(G.walk_spec(area, 0))
    out = []
    for stop in (0, 1):
        found, at = {}, 0
        for key, typ, off, size in tags:
            if typ == "Z" and key in ("RG", "SA") and key not in found:
                found[key] = (off, size)
                if stop and key == "RG":
                    at = off + size + 1
                    break
        outcome = "AT_RG" if stop and "RG" in found else "END"
        rg, sa = found.get("RG", (0, 0)), found.get("SA", (0, 0))
        out.append("T %s %d %s %d %d %d %d %d %d %d %s" % (label, stop, outcome, at, "RG" in found, rg[0], rg[1], "SA" in found, sa[0], sa[1],
                                                             area.hex() or "-"))
    return out


def fixture_text():
    lines = []
    records = G.evidence_records()
    for k, rec in enumerate(records):
        body = bw.encode_record(rec)[0][4:]
        if rec["name"] in WHOLE_RECORDS:
            lines.append("R %s %d %s" % (rec["name"], G.tag_area(body), body.hex()))
        if rec["cigar"] == "60M40S" or k >= 2 * 15:                # every split candidate, and the plain reads of the last decorations
            lines += _area_lines(rec["name"], body[G.tag_area(body):])
    lines += _area_lines("no_tags", b"")
    bad = bw.encode_record(dict(records[0], tags=[G.UNKNOWN_SUBTYPE, ("RG", "Z", "rg")]))[0][4:]
    lines += ["T unknown_subtype %d MALFORMED 0 0 0 0 0 0 0 %s" % (stop, bad[G.tag_area(bad):].hex()) for stop in (0, 1)]
    for text in sorted({c for c, _pos, _sa in G.CIGARS} | {sa.split(",")[3] for sa in (G.REAL_SA, G.FAKE_SA)} | {"3M"}):
        ops = bw.parse_cigar(text)
        total = lambda which: sum(n for op, n in ops if bw.CIGAR_OPS[op] in which)
        lines.append("C %s %d %d %d %d" % (text, len(ops), total("MI=X"), total("SH"), total("MDN=X")))
    return "\n".join(lines) + "\n"


def test_the_fixture_is_the_corpus():
    assert open(FIXTURE).read() == fixture_text()
    assert sum(1 for l in fixture_text().split("\n") if l.startswith("R ")) == len(WHOLE_RECORDS)


def test_record_rules_under_asan_and_ubsan(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_record_rules")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_record_rules_main.cpp"), "-o", exe]
    # the runtime linked into the program where this g++ has the static one: the program then starts whatever else the
    # environment makes the loader map in front of it
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, FIXTURE], env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    n_areas, n_records, n_cigars = (int(lines[-2].split(", ")[k].split()[0]) for k in range(3))
    text = open(FIXTURE).read().split("\n")
    assert (n_areas, n_records, n_cigars) == tuple(sum(1 for l in text if l.startswith(c)) for c in ("T ", "R ", "C "))


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        f.write(fixture_text())

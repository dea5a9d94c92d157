"""svtyper_amd.update_info on the host: every case of tests/updateinfocases.py against what the reference's scripts/update_info.py
gave for it (tests/golden/update_info_cases.json.gz, made by tests/golden/make_golden_update_info.py): the bytes, or the status,
the exception, the message and the bytes written before it; the number of lines the plain C++ computed; the order of the SQ sum;
blocks; the command line."""
import gzip
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import tbxcases as X
import updateinfocases as K

from svtyper_amd import native_reads as nr
from svtyper_amd import update_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
with gzip.open(os.path.join(ROOT, "tests", "golden", "update_info_cases.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["name"]: c for c in GOLDEN["cases"]}


def run(case, tmp_path, sink=None, **options):
    """`sink`: where the text goes (what was written before an error stays readable there)"""
    out, stats = sink if sink is not None else io.StringIO(), {}
    update_info.update_info(K.write_case(case, str(tmp_path)), vcf_out=out, file_date=GOLDEN["file_date"], stats=stats, **options)
    return out.getvalue(), stats


def records(stats):
    return np.concatenate(stats["results"]) if stats["results"] else np.zeros(0, nr.UPDATE_INFO_LINE)


def sq_of(line):
    """the SQ of the positive samples of a body line of the corpus, in sample order"""
    columns = [c.split(":") for c in line.rstrip("\n").split("\t")[9:]]
    return [float(c[2]) for c in columns if c[0] not in ("0/0", "./.")]


def strided(values, lanes=256):
    """the sum a tree of `lanes` partials gives: what sum_sq must NOT be"""
    partial = [0.0] * lanes
    for s, v in enumerate(values):
        partial[s % lanes] += v
    while len(partial) > 1:
        partial = [a + b for a, b in zip(partial[::2], partial[1::2])]
    return partial[0]


def test_corpus_is_the_goldens():
    """the goldens were made from this very corpus; every width, every outcome and the lines whose sum depends on its order are there"""
    assert [c["name"] for c in CASES] == [c["name"] for c in GOLDEN["cases"]]
    for case in CASES:
        assert (EXPECTED[case["name"]]["expected"]["status"] != 0) == (case["error"] is not None), case["name"]
    assert {c["n_samples"] for c in CASES} >= {0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097}
    assert K.CAPACITY == nr.UPDATE_INFO_CAPACITY
    kinds = {EXPECTED[c["name"]]["expected"]["exception"] for c in CASES if c["error"] is not None}
    assert kinds == {"ValueError", "KeyError", "IndexError", "UnboundLocalError", None}
    messages = {EXPECTED[c["name"]]["expected"]["stderr"] for c in CASES if c["error"] is not None}
    assert messages == {"", update_info.FORMAT_MESSAGE % "XX", update_info.COLUMNS_MESSAGE}
    assert any(c["error"] is not None and EXPECTED[c["name"]]["expected"]["stdout"].count("\n1\t") == 1 for c in CASES)
    big, bits = [l for l in next(c for c in CASES if c["name"] == "msq_order_matters")["vcf"].splitlines() if not l.startswith("#")]
    in_order = sum(sq_of(big), 0.0)
    assert in_order == 1e15 and strided(sq_of(big)) > 1e15 + 1
    assert "%0.2f" % (in_order / 300) != "%0.2f" % (strided(sq_of(big)) / 300)    # the output text itself tells the two orders apart
    in_order, tree = sum(sq_of(bits), 0.0), strided(sq_of(bits))
    assert in_order != tree and abs(in_order - tree) <= 64 * np.spacing(in_order)  # ... and the records' bits do, in the last places
    assert min(sq_of(bits)) < 1 and max(sq_of(bits)) > 1e5
    whole = "".join(e["expected"].get("stdout", "") for e in GOLDEN["cases"])
    assert all(word in whole for word in ("MSQ=.\t", "AF=True", "\t\t\n", ";PE;", "MSQ=0.12\t", "MSQ=0.38\t", "\t0.00\t", ":.:.\t")) and "SNAME" not in whole


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_engine_gives_the_reference_bytes(case, tmp_path):
    golden = EXPECTED[case["name"]]["expected"]
    if case["error"] is not None:
        written = io.StringIO()
        with pytest.raises(update_info.UpdateInfoError) as e:
            run(case, tmp_path, sink=written)
        assert e.value.line == case["error"] and os.path.basename(e.value.file) == "cohort.vcf"
        assert written.getvalue() == golden["stdout"]               # the lines in front of the one the script dies on
        assert e.value.reference == golden["exception"]
        assert (e.value.verbatim or "") == golden["stderr"]
        return
    text, stats = run(case, tmp_path)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"]                # the corpus meets what it says of itself
    recs = records(stats)
    assert ((recs["flags"] != 0) == (recs["route"] == nr.UPDATE_INFO_PLAIN)).all() and int((recs["flags"] != 0).sum()) == case["slow_lines"]
    body = [l for l in case["vcf"].splitlines() if not l.startswith("#")]
    assert stats["lines"] == len(body) == len(recs)
    if case["name"] == "msq_order_matters":                         # sum_sq is the sum in sample order, bit for bit
        for rec, line in zip(recs, body):
            assert rec["sum_sq"] == np.float64(sum(sq_of(line), 0.0)).view(np.uint64) and rec["num_pos"] == 300


@pytest.mark.parametrize("case", K.departure_cases(), ids=[c["name"] for c in K.departure_cases()])
def test_stated_departures_are_refused(case, tmp_path):
    with pytest.raises(update_info.UpdateInfoError) as e:
        run(case, tmp_path)
    assert e.value.line == case["error"] and e.value.reference is None and e.value.verbatim is None
    assert ("not finite" if case["kind"] == "NONFINITE" else "beyond 64 bits") in str(e.value)


def test_an_error_names_the_sample_and_the_token(tmp_path):
    case = next(c for c in CASES if c["name"] == "error_sq_no_number")
    with pytest.raises(update_info.UpdateInfoError) as e:
        run(case, tmp_path)
    assert (e.value.sample, e.value.token) == ("S0003", "1.5x") and "sample S0003" in str(e.value) and "1.5x" in str(e.value)
    case = next(c for c in CASES if c["name"] == "error_missing_sample_column")
    with pytest.raises(update_info.UpdateInfoError) as e:
        run(case, tmp_path)
    assert (e.value.sample, e.value.token) == ("S0003", "AP")


@pytest.mark.parametrize("name", ["width_65", "qual_and_pos", "last_line_bare", "format_short_sample_columns", "msq_order_matters", "error_ap_dot"])
def test_three_blocks_give_the_same_bytes(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    body = [l for l in case["vcf"].splitlines(True) if not l.startswith("#")]
    if case["error"] is not None:
        written = io.StringIO()
        with pytest.raises(update_info.UpdateInfoError) as e:
            run(case, tmp_path, sink=written, block_bytes=1)
        assert e.value.line == case["error"] and written.getvalue() == EXPECTED[name]["expected"]["stdout"]
        return
    whole, one = run(case, tmp_path)
    text, stats = run(case, tmp_path, block_bytes=sum(map(len, body)) // 3 + 1)
    assert one["blocks"] == 1 and stats["blocks"] >= min(3, len(body)) and text == whole == EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"] and records(stats).tobytes() == records(one).tobytes()
    text, stats = run(case, tmp_path, block_bytes=1)                # a line at the least
    assert stats["blocks"] == len(body) and text == whole


def test_gzipped_input_by_name_by_content_and_as_an_open_file(tmp_path):
    case = next(c for c in CASES if c["name"] == "info_items")
    vcf = K.write_case(case, str(tmp_path))
    for path in (vcf + ".gz", str(tmp_path / "no_suffix")):
        with open(vcf, "rb") as f, gzip.open(path, "wb") as z:
            z.write(f.read())
    want = EXPECTED["info_items"]["expected"]["stdout"]
    for source in (vcf + ".gz", str(tmp_path / "no_suffix")):
        out = io.StringIO()
        update_info.update_info(source, vcf_out=out, file_date=GOLDEN["file_date"])
        assert out.getvalue() == want
    for path in (vcf, str(tmp_path / "no_suffix")):
        out = io.StringIO()
        with open(path, "rb") as f:                                 # (buffered: it can peek)
            update_info.update_info(f, vcf_out=out, file_date=GOLDEN["file_date"])
        assert out.getvalue() == want


def test_keep_contigs_places_the_lines_before_chrom(tmp_path):
    case = next(c for c in CASES if c["name"] == "width_1")
    plain, _s = run(case, tmp_path)
    kept, _s = run(case, tmp_path, keep_contigs=True)
    lines = kept.splitlines()
    at = next(k for k, l in enumerate(lines) if l.startswith("#CHROM"))
    assert lines[at - 1] == "##contig=<ID=1,length=249250621>" and "##contig" not in plain
    assert [l for l in lines if not l.startswith("##contig")] == plain.splitlines()


def command(case, tmp_path, more, stdin=False):
    vcf = K.write_case(case, str(tmp_path))
    cmd = [sys.executable, "-m", "svtyper_amd.update_info"] + ([] if stdin else [vcf]) + more
    if stdin:
        with open(vcf, "rb") as f:
            return subprocess.run(cmd, stdin=f, capture_output=True, cwd=ROOT, timeout=120)
    return subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=120)


def dated(text):
    """(the command line has no file_date: the line is the clock's)"""
    return "\n".join(("##fileDate=" + GOLDEN["file_date"]) if l.startswith("##fileDate=") else l for l in text.split("\n"))


@pytest.mark.parametrize("name,stdin", [("info_items", False), ("format_short_sample_columns", True), ("error_undeclared_format_key", False),
                                        ("error_seven_columns", True), ("error_ap_dot", False)])
def test_command_line(name, stdin, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    golden = EXPECTED[name]["expected"]
    r = command(case, tmp_path, [], stdin)
    assert r.returncode == golden["status"], r.stderr
    assert dated(r.stdout.decode()) == golden["stdout"]             # with an error: the lines in front of it
    if golden["status"] and golden["stderr"]:
        assert r.stderr.decode() == golden["stderr"]
    elif golden["status"]:
        assert r.stderr.decode().startswith("Error: ") and ", line %d" % case["error"] in r.stderr.decode()


def test_command_line_to_a_sorted_indexed_bgzf_file(tmp_path):
    case = next(c for c in CASES if c["name"] == "width_65")
    out = str(tmp_path / "updated.vcf.gz")
    r = command(case, tmp_path, ["--keep-contigs", "--bgzf", "--sort", "--tabix", "-o", out])
    assert r.returncode == 0, r.stderr
    kept = io.StringIO()
    update_info.update_info(K.write_case(case, str(tmp_path)), vcf_out=kept, file_date=GOLDEN["file_date"], keep_contigs=True)
    assert [l for l in kept.getvalue().splitlines() if not l.startswith("##contig")] == EXPECTED["width_65"]["expected"]["stdout"].splitlines()
    raw = open(out, "rb").read()
    members = X.Members(raw)
    assert dated(members.text().decode()).encode() == X.sorted_text(kept.getvalue().encode())
    assert [l.split("\t")[1] for l in members.text().decode().splitlines() if not l.startswith("#")] == ["1000", "2000", "3000"]
    tbi = X.read_tbi(open(out + ".tbi", "rb").read())
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(members.text(), n_random=50), members)

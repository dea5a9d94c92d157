"""svtyper_amd.classify on the host: every case of tests/classifycases.py against what the reference's scripts/sv_classifier.py
gave for it (tests/golden/classify_cases.json.gz, made by tests/golden/make_golden_classify.py): the bytes, or the status, the
exception and the message; the regression's slope and r against the scipy values the generator recorded; the medians against
numpy, bit for bit; the band around the thresholds; blocks; the command line."""
import gzip
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import classifycases as K
import tbxcases as X

from svtyper_amd import classify
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
with gzip.open(os.path.join(ROOT, "tests", "golden", "classify_cases.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["name"]: c for c in GOLDEN["cases"]}
BAND = 1e-9                                         # of SVT_CLASSIFY_NEAR, and of the records against scipy


def run(case, tmp_path, sink=None, **options):
    """`sink`: where the text goes (what was written before an error stays readable there)"""
    vcf, gender, exclude, annotation = K.write_case(case, str(tmp_path))
    out, stats = sink if sink is not None else io.StringIO(), {}
    classify.classify(vcf, gender, exclude, annotation, vcf_out=out, file_date=GOLDEN["file_date"], stats=stats, **case["options"], **options)
    return out.getvalue(), stats


def records(stats):
    return np.concatenate(stats["results"]) if stats["results"] else np.zeros(0, nr.CLASSIFY_LINE)


def bits(value):
    return np.float64(value).view(np.uint64)


def test_corpus_is_the_goldens():
    """the goldens were made from this very corpus; every width and every outcome is there"""
    assert [c["name"] for c in CASES] == [c["name"] for c in GOLDEN["cases"]]
    for case in CASES:
        assert (EXPECTED[case["name"]]["expected"]["status"] != 0) == (case["error"] is not None), case["name"]
    assert {c["n_samples"] for c in CASES} >= set(K.SAMPLE_COUNTS) | {K.CAPACITY + 1}
    assert K.CAPACITY == nr.CLASSIFY_CAPACITY
    kinds = {EXPECTED[c["name"]]["expected"]["exception"] for c in CASES if c["error"] is not None}
    assert kinds == {"ValueError", "KeyError", "IndexError", None}
    # the median's two middle values in different strides of the kernel's 256 lanes, and different
    stride = next(c for c in CASES if c["name"] == "low_middle_in_two_strides")
    columns = stride["vcf"].splitlines()[-1].split("\t")[9:]
    refs = sorted((float(c.split(":")[1]), s) for s, c in enumerate(columns) if c.split(":")[0] == "0/0")
    (a, sa), (b, sb) = refs[len(refs) // 2 - 1], refs[len(refs) // 2]
    assert len(refs) % 2 == 0 and a != b and sa // 256 != sb // 256
    assert [v for v, _s in refs].count(a) == 1 and [v for v, _s in refs].count(b) == 1
    assert any(c["annotation"] is not None and c["error"] is not None and c["vcf"].count("\n") > c["error"] for c in CASES)
    whole = "".join(e["expected"].get("stdout", "") for e in GOLDEN["cases"] if e["expected"]["status"] == 0)
    assert all(word in whole for word in ("SVTYPE=BND", "SVTYPE=MEI", "SVTYPE=DEL", "SVTYPE=DUP", "<DEL:ME:", "SECONDARY=True", "SU=True"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_engine_gives_the_reference_bytes(case, tmp_path):
    golden = EXPECTED[case["name"]]
    if case["error"] is not None:
        written = io.StringIO()
        with pytest.raises(classify.ClassifyError) as e:
            run(case, tmp_path, sink=written)
        assert e.value.line == case["error"] and os.path.basename(e.value.file) == "cohort.vcf"
        assert written.getvalue() == golden["expected"]["stdout"]   # the lines in front of the one the script dies on
        assert e.value.reference == golden["expected"]["exception"]
        assert (e.value.verbatim or "") == golden["expected"]["stderr"]
        return
    text, stats = run(case, tmp_path)
    assert text == golden["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]                # the corpus meets what it says of itself
    recs = records(stats)
    # no golden case sits near a threshold: the goldens hold whatever the order of the sums
    assert stats["near_lines"] == 0 and not (recs["flags"] & nr.CLASSIFY_NEAR).any()
    # the regressions the script ran, in its order
    ran = recs[(recs["route"] == nr.CLASSIFY_HIGH) & ((recs["slope"] != 0) | (recs["r2"] != 0))]
    assert len(ran) == len(golden["regressions"])
    for rec, (slope, r) in zip(ran, golden["regressions"]):
        print(case["name"], "slope", rec["slope"], slope, "r", math.copysign(math.sqrt(rec["r2"]), rec["slope"]), r)
        assert abs(rec["slope"] - slope) <= BAND * abs(slope)
        assert abs(math.copysign(math.sqrt(rec["r2"]), rec["slope"]) - r) <= BAND * abs(r)
    # the medians of the low-frequency test against numpy, bit for bit
    for at, values in case["low"].items():
        rec = recs[at]
        assert rec["route"] == nr.CLASSIFY_LOW and rec["n_ref"] == len(values), at
        median = np.median(values) if values else 0.0
        mad = np.median(np.abs(np.array(values) - median)) if values else 0.0
        assert bits(rec["median"]) == bits(median) and bits(rec["mad"]) == bits(mad), (at, rec["median"], median, rec["mad"], mad)


def test_a_regression_on_its_threshold_is_flagged_near(tmp_path):
    """CN = 2 - AB exactly: the DEL's signed slope is the default threshold of 1 (or within a rounding of it)"""
    text, stats = run(K.near_case(), tmp_path)
    rec = records(stats)[0]
    assert rec["route"] == nr.CLASSIFY_HIGH and abs(rec["slope"] + 1.0) <= BAND
    assert rec["flags"] & nr.CLASSIFY_NEAR and stats["near_lines"] == 1
    assert ("SVTYPE=DEL" in text) == bool(rec["verdict"])           # the verdict is still the rule's
    _text, far = run(dict(K.near_case(), options=dict(K.OPTIONS, slope_threshold=1.001)), tmp_path)
    assert far["near_lines"] == 0 and not records(far)[0]["verdict"]


@pytest.mark.parametrize("case", K.nonfinite_cases(), ids=[c["name"] for c in K.nonfinite_cases()])
def test_nan_and_inf_are_refused(case, tmp_path):
    with pytest.raises(classify.ClassifyError) as e:
        run(case, tmp_path)
    assert e.value.line == case["error"] and e.value.reference is None and "not finite" in str(e.value)


@pytest.mark.parametrize("name", ["width_65", "annotation", "last_line_verbatim_bare", "last_line_rewritten_bare", "qual_and_pos", "error_cn_no_number"])
def test_three_blocks_give_the_same_bytes(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    body = [l for l in case["vcf"].splitlines(True) if not l.startswith("#")]
    if case["error"] is not None:
        with pytest.raises(classify.ClassifyError) as e:
            run(case, tmp_path, block_bytes=1)
        assert e.value.line == case["error"]
        return
    text, stats = run(case, tmp_path, block_bytes=sum(map(len, body)) // 3 + 1)
    assert stats["blocks"] >= 3 and text == EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]
    text, stats = run(case, tmp_path, block_bytes=1)                # a line at the least
    assert stats["blocks"] == len(body) and text == EXPECTED[name]["expected"]["stdout"]


def test_gzipped_input_and_open_files(tmp_path):
    case = next(c for c in CASES if c["name"] == "annotation")
    vcf, gender, _exclude, annotation = K.write_case(case, str(tmp_path))
    for path in (vcf, annotation):
        with open(path, "rb") as f, gzip.open(path + ".gz", "wb") as z:
            z.write(f.read())
    out = io.StringIO()
    with open(gender) as g:
        classify.classify(vcf + ".gz", g, annotation=annotation + ".gz", vcf_out=out, file_date=GOLDEN["file_date"])
    assert out.getvalue() == EXPECTED["annotation"]["expected"]["stdout"]


def test_keep_contigs_places_the_lines_before_chrom(tmp_path):
    case = next(c for c in CASES if c["name"] == "width_9")
    plain, _s = run(case, tmp_path)
    kept, _s = run(case, tmp_path, keep_contigs=True)
    lines = kept.splitlines()
    at = next(k for k, l in enumerate(lines) if l.startswith("#CHROM"))
    assert lines[at - 1] == "##contig=<ID=1,length=249250621>" and "##contig" not in plain
    assert [l for l in lines if not l.startswith("##contig")] == plain.splitlines()


def command(case, tmp_path, more):
    vcf, gender, exclude, annotation = K.write_case(case, str(tmp_path))
    cmd = [sys.executable, "-m", "svtyper_amd.classify", "-i", vcf, "-g", gender] + (["-e", exclude] if exclude else [])
    cmd += (["-a", annotation] if annotation else []) + ["-f", str(case["options"]["f_overlap"]), "-s", str(case["options"]["slope_threshold"]),
                                                         "-r", str(case["options"]["rsquared_threshold"])]
    return subprocess.run(cmd + more, capture_output=True, text=True, cwd=ROOT, timeout=120)


def dated(text):
    """(the command line has no file_date: the line is the clock's)"""
    return "\n".join(("##fileDate=" + GOLDEN["file_date"]) if l.startswith("##fileDate=") else l for l in text.split("\n"))


@pytest.mark.parametrize("name", ["annotation_fraction_0.5", "high_low_slope_threshold", "switch_10_one_excluded", "error_undeclared_format_key",
                                  "error_bnd_without_end"])
def test_command_line(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    golden = EXPECTED[name]["expected"]
    r = command(case, tmp_path, [])
    assert r.returncode == golden["status"], r.stderr
    if golden["status"] == 0:                       # (without -e the script ends in an AttributeError behind this output; here: 0)
        assert dated(r.stdout) == golden["stdout"]
    elif golden["stderr"]:
        assert r.stderr == golden["stderr"]
    else:
        assert r.stderr.startswith("Error: ") and "cohort.vcf, line %d" % case["error"] in r.stderr


def test_command_line_to_a_sorted_indexed_bgzf_file(tmp_path):
    case = next(c for c in CASES if c["name"] == "width_65")
    out = str(tmp_path / "classified.vcf.gz")
    r = command(case, tmp_path, ["--bgzf", "--sort", "--tabix", "-o", out])
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    members = X.Members(raw)
    assert dated(members.text().decode()).encode() == X.sorted_text(EXPECTED["width_65"]["expected"]["stdout"].encode())
    tbi = X.read_tbi(open(out + ".tbi", "rb").read())
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(members.text(), n_random=50), members)

"""svtyper_amd.paste on the host: every case of tests/pastecases.py against what the reference's scripts/vcf_paste.py and
scripts/vcf_allele_freq.py gave for it (tests/golden/paste_cases.json.gz, made by tests/golden/make_golden_paste.py), from Python
and through the command line; the options the reference does not have; the usage errors."""
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

import pastecases as P

from svtyper_amd import paste

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = P.cases()
with gzip.open(os.path.join(ROOT, "tests", "golden", "paste_cases.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["name"]: c for c in GOLDEN["cases"]}


def run(case, tmp_path, **options):
    master, paths = P.write_case(case, str(tmp_path))
    out, stats = io.StringIO(), {}
    paste.paste(paths, master=master, vcf_out=out, file_date=GOLDEN["file_date"], stats=stats, **P.case_options(case), **options)
    return out.getvalue(), stats, master, paths


def test_corpus_is_the_goldens():
    """the goldens were made from these very inputs; every count of inputs and every kind of case is there"""
    assert [c["name"] for c in CASES] == [c["name"] for c in GOLDEN["cases"]]
    for case in CASES:
        golden = EXPECTED[case["name"]]
        assert all(case[k] == golden[k] for k in ("master", "inputs", "sum_quals", "afreq")), case["name"]
        assert (golden["expected"]["status"] != 0) == (case["error"] is not None), case["name"]
        if case["error"]:
            assert bool(golden["expected"]["stderr"]) == case["error"]["message"], case["name"]
    assert {len(c["inputs"]) for c in CASES} == set(P.INPUT_COUNTS)
    assert {(c["master"] is None, c["sum_quals"]) for c in CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert all(5 <= c["inputs"][0].count("\n") - 2 <= 40 or c["master"] is None for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_engine_gives_the_reference_bytes(case, tmp_path):
    golden = EXPECTED[case["name"]]["expected"]
    if case["error"] is None:
        text, stats, _master, _paths = run(case, tmp_path)
        assert text == golden["stdout"]
        assert stats["host_lines"] == case["slow_lines"]            # the corpus meets what it says of itself
        return
    with pytest.raises(paste.PasteError) as e:
        run(case, tmp_path)
    names = ["master.vcf"] + ["in%03d.vcf" % k for k in range(len(case["inputs"]))]
    assert os.path.basename(e.value.file) == names[case["error"]["file"]]
    assert e.value.line == case["error"]["line"]
    assert (e.value.verbatim == golden["stderr"]) if case["error"]["message"] else e.value.verbatim is None


@pytest.mark.parametrize("name", ["n3_afreq_shapes_q", "n2_master_q_tenths", "n3_short_input", "n2_qual_no_number"])
def test_command_line(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    golden = EXPECTED[name]["expected"]
    master, paths = P.write_case(case, str(tmp_path))
    listing = tmp_path / "list.txt"
    listing.write_text("".join(p + "\n" for p in paths))
    out = tmp_path / "out.vcf"
    cmd = [sys.executable, "-m", "svtyper_amd.paste", "-f", str(listing), "-o", str(out)]
    cmd += (["-m", master] if master else []) + (["-q"] if case["sum_quals"] else []) + (["--afreq"] if case["afreq"] else [])
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == golden["status"], r.stderr
    if golden["status"] == 0:
        text = out.read_text()
        if case["afreq"]:                           # (the command line has no file_date: the line is the clock's)
            text = "\n".join(("##fileDate=" + GOLDEN["file_date"]) if l.startswith("##fileDate=") else l for l in text.split("\n"))
        assert text == golden["stdout"]
    elif golden["stderr"]:
        assert r.stderr == golden["stderr"]
    else:
        assert r.stderr.startswith("Error: ") and os.path.basename(paths[case["error"]["file"] - 1]) in r.stderr


def test_gzipped_inputs_are_read_through_gzip(tmp_path):
    case = next(c for c in CASES if c["name"] == "n3_afreq_shapes")
    master, paths = P.write_case(case, str(tmp_path))
    zipped = []
    for p in paths:
        with open(p, "rb") as f, gzip.open(p + ".gz", "wb") as z:
            z.write(f.read())
        zipped.append(p + ".gz")
    out = io.StringIO()
    paste.paste(zipped, master=master, vcf_out=out, afreq=True, file_date=GOLDEN["file_date"])
    assert out.getvalue() == EXPECTED[case["name"]]["expected"]["stdout"]


@pytest.mark.parametrize("name", ["n3_afreq_shapes_q", "n65_slow_second_stride", "n130_plain_q"])
def test_three_blocks_give_the_same_bytes(name, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    row = sum(len(t.splitlines()[-1]) + 1 for t in case["inputs"]) + 400
    text, stats, _m, _p = run(case, tmp_path, block_bytes=2 * row)
    assert stats["blocks"] >= 3
    assert text == EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]
    text, stats, _m, _p = run(case, tmp_path, block_bytes=1)       # a line of every file at the least
    assert stats["blocks"] == stats["lines"] and text == EXPECTED[name]["expected"]["stdout"]


def unsafe_case():
    """n3_forty_lines with the POS of line 18 changed in input 1"""
    case = dict(next(c for c in CASES if c["name"] == "n3_forty_lines"))
    lines = case["inputs"][1].splitlines(True)
    columns = lines[2 + 17].split("\t")
    columns[1] = str(int(columns[1]) + 1)
    lines[2 + 17] = "\t".join(columns)
    case["inputs"] = [case["inputs"][0], "".join(lines), case["inputs"][2]]
    return case


def test_safe_names_file_line_and_field(tmp_path):
    case = unsafe_case()
    text, _stats, _m, _p = run(case, tmp_path)                      # the default joins by line number alone, as the reference does
    assert text == EXPECTED["n3_forty_lines"]["expected"]["stdout"]
    for block_bytes in (None, 4000):
        with pytest.raises(paste.PasteError) as e:
            run(case, tmp_path, safe=True, block_bytes=block_bytes)
        assert (os.path.basename(e.value.file), e.value.line, e.value.field) == ("in001.vcf", 2 + 18, "POS")
    text, _stats, _m, _p = run(next(c for c in CASES if c["name"] == "n3_forty_lines"), tmp_path, safe=True)
    assert text == EXPECTED["n3_forty_lines"]["expected"]["stdout"]


def test_keep_contigs_places_the_lines_before_chrom(tmp_path):
    case = next(c for c in CASES if c["name"] == "n3_afreq_contigs")
    contigs = [l for l in case["master"].splitlines() if l.startswith("##contig")]
    assert len(contigs) >= 2
    plain, _s, _m, _p = run(case, tmp_path)
    assert "##contig" not in plain                                  # the reference's bytes: the lines are dropped
    kept, _s, _m, _p = run(case, tmp_path, keep_contigs=True)
    lines = kept.splitlines()
    at = next(k for k, l in enumerate(lines) if l.startswith("#CHROM"))
    assert lines[at - len(contigs):at] == contigs
    assert [l for l in lines if not l.startswith("##contig")] == plain.splitlines()


@pytest.mark.parametrize("options, words", [(["--bcf", "--bgzf"], "two formats for one output"), (["--bcf", "--tabix"], "--tabix indexes VCF text"),
                                            (["--bgzf", "--csi", "--tabix"], "two formats for one index")])
def test_option_conflicts_are_usage_errors(options, words, tmp_path):
    listing = tmp_path / "list.txt"
    listing.write_text("")
    r = subprocess.run([sys.executable, "-m", "svtyper_amd.paste", "-f", str(listing), "-o", str(tmp_path / "out")] + options, capture_output=True,
                       text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and words in r.stderr


def test_bcf_output_needs_the_contigs(tmp_path):
    """--afreq drops the ##contig lines as the reference does, and the BCF writer refuses a record of an undeclared contig;
    with --keep-contigs the same run is a sorted, indexed BCF"""
    from svtyper_amd import bcf_out
    case = next(c for c in CASES if c["name"] == "n3_afreq_contigs")
    master, paths = P.write_case(case, str(tmp_path))
    for keep in (False, True):
        path = str(tmp_path / ("kept.bcf" if keep else "dropped.bcf"))
        out = bcf_out.open_bcf(path, sort=True, index="csi")
        paste.paste(paths, master=master, vcf_out=out, file_date=GOLDEN["file_date"], keep_contigs=keep, **P.case_options(case))
        if keep:
            out.close()
            assert os.path.getsize(path) > 28 and os.path.getsize(path + ".csi") > 28
        else:
            with pytest.raises(bcf_out.BcfError):
                out.close()

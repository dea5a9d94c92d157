"""svtyper_amd.modify_header: every case of tests/modifyheadercases.py against what the reference's scripts/vcf_modify_header.py
gave for it (tests/golden/modify_header_cases.json.gz, made by tests/golden/make_golden_modify_header.py); the body copied
verbatim; --keep-contigs; gzip input; the command line."""
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

import modifyheadercases as K

from svtyper_amd import modify_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
with gzip.open(os.path.join(ROOT, "tests", "golden", "modify_header_cases.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["name"]: c for c in GOLDEN["cases"]}
OPTIONS = ("vcf_id", "category", "type", "number", "description")


def run(case, source, **more):
    out = io.BytesIO()
    modify_header.modify_header(source, out, *[case[k] for k in OPTIONS], file_date=GOLDEN["file_date"], **more)
    return out.getvalue()


def test_corpus_is_the_goldens():
    assert [c["name"] for c in CASES] == [c["name"] for c in GOLDEN["cases"]]
    whole = "".join(e["expected"].get("stdout", "") for e in GOLDEN["cases"])
    for word in ('##FILTER=<ID=ODD,Description="a > inside, and a comma">', '##INFO=<ID=Q,Number=.,Type=String,Description="quoted">',
                 "##INFO=<ID=X,Number=None,Type=None,Description=\"None\">", "INFO\n", "not parsed\n\n#late\t\n"):
        assert word in whole, word
    assert EXPECTED["no_body"]["expected"]["stdout"] == "" and EXPECTED["error_no_chrom_line"]["expected"]["exception"] == "UnboundLocalError"
    replaced = EXPECTED["info_replaces"]["expected"]["stdout"].splitlines()
    assert [l for l in replaced if l.startswith("##INFO")][-1] == '##INFO=<ID=END,Number=1,Type=Integer,Description="End, declared anew">'
    assert sum(l.startswith("##INFO=<ID=END,") for l in replaced) == 1


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_reference_bytes(case, tmp_path):
    golden = EXPECTED[case["name"]]["expected"]
    path = K.write_case(case, str(tmp_path))
    if golden["status"]:
        with pytest.raises(modify_header.ModifyHeaderError) as e:
            run(case, path)
        assert e.value.reference == golden["exception"] and golden["stdout"] == ""
        return
    got = run(case, path)
    assert got == golden["stdout"].encode()
    body = case["vcf"][case["vcf"].index("\n", case["vcf"].index("#CHROM")) + 1:]
    assert got.endswith(body.encode()) or not body                  # the body verbatim, blanks and all


def test_keep_contigs_and_gzip_input(tmp_path):
    case = next(c for c in CASES if c["name"] == "info_new")
    path = K.write_case(case, str(tmp_path))
    plain = run(case, path).decode()
    kept = run(case, path, keep_contigs=True).decode().split("\n")
    at = next(k for k, l in enumerate(kept) if l.startswith("#CHROM"))
    assert kept[at - 1] == "##contig=<ID=1,length=249250621>" and "##contig" not in plain
    assert [l for l in kept if not l.startswith("##contig")] == plain.split("\n")
    with open(path, "rb") as f, gzip.open(path + ".gz", "wb") as z:
        z.write(f.read())
    assert run(case, path + ".gz").decode() == plain
    with open(path, "rb") as f:
        assert run(case, f).decode() == plain


@pytest.mark.parametrize("name,stdin", [("info_new", False), ("filter_new", True), ("normalise_only", False), ("error_no_chrom_line", False)])
def test_command_line(name, stdin, tmp_path):
    case = next(c for c in CASES if c["name"] == name)
    golden = EXPECTED[name]["expected"]
    vcf = K.write_case(case, str(tmp_path))
    flags = dict(vcf_id="-i", category="-c", type="-t", number="-n", description="-d")
    cmd = [sys.executable, "-m", "svtyper_amd.modify_header"] + [w for k in OPTIONS if case[k] is not None for w in (flags[k], case[k])]
    if stdin:
        with open(vcf, "rb") as f:
            r = subprocess.run(cmd, stdin=f, capture_output=True, cwd=ROOT, timeout=120)
    else:
        r = subprocess.run(cmd + [vcf, "-o", str(tmp_path / "out.vcf")], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == golden["status"], r.stderr
    text = r.stdout if stdin else open(str(tmp_path / "out.vcf"), "rb").read()
    today = "\n".join(("##fileDate=" + GOLDEN["file_date"]) if l.startswith("##fileDate=") else l for l in text.decode().split("\n"))
    assert today == golden["stdout"]
    if golden["status"]:
        assert r.stderr.decode().startswith("Error: ")

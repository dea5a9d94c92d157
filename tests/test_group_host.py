"""svtyper_amd.group_multiline on the host: every case of tests/groupcases.py against what the reference's
scripts/vcf_group_multiline.py gave for it (tests/golden/group_cases.json.gz, made by tests/golden/make_golden_group.py): the
bytes, or the status, the exception, the message and the bytes written before it; the lines the plain C++ decided; the plan; and
a plain-Python restatement of "regular" and of the closed form of DESIGN 3.4, checked against the script's sequential dictionary."""
import gzip
import io
import json
import os
import random
import re
import subprocess
import sys

import pytest

import groupcases as K
import tbxcases as X

from svtyper_amd import bcf_in, bcf_out, group_multiline
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.cases()
with gzip.open(os.path.join(ROOT, "tests", "golden", "group_cases.json.gz"), "rt") as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["name"]: c for c in GOLDEN["cases"]}


def run(case, tmp_path, sink=None, **options):
    """`sink`: where the text goes (what was written before an error stays readable there)"""
    out, stats = sink if sink is not None else io.StringIO(), {}
    group_multiline.group_multiline(K.write_case(case, str(tmp_path)), vcf_out=out, file_date=GOLDEN["file_date"], stats=stats, **options)
    return out.getvalue(), stats


# ---- the restatement: a file is a list of (is_bnd, id, mateid or None)
def read(case):
    """the body lines of a case in front of its error, as the join sees them (the script's split('=') included)"""
    lines = case["vcf"].splitlines()
    head = sum(1 for l in lines if l.startswith("#"))
    out = []
    for l in lines[head:case["error"] - 1 if case["error"] is not None else None]:
        v = l.rstrip().split("\t")
        info = {}
        for item in v[7].split(";"):
            parts = item.split("=")
            info[parts[0]] = parts[1] if len(parts) > 1 else True
        out.append((info["SVTYPE"] == "BND", v[2], info.get("MATEID") if info.get("MATEID") is not True else None))
    return out


def sequential(lines):
    """the script's loop: (line, source) in output order"""
    stored, plan = {}, []
    for i, (bnd, ident, mate) in enumerate(lines):
        if not bnd:
            plan.append((i, i))
        elif mate is not None and mate in stored:
            plan += [(stored[mate], stored[mate]), (i, stored[mate])]
        else:
            stored[ident] = i
    return plan


def mates(lines):
    """mate[i]: the BND line whose ID is i's MATEID (the last such line), or None"""
    by_id = {ident: i for i, (bnd, ident, _m) in enumerate(lines) if bnd}
    return [by_id.get(mate) if bnd and mate is not None else None for bnd, _i, mate in lines]


def regular(lines):
    ids = [ident for bnd, ident, _m in lines if bnd]
    if len(set(ids)) != len(ids):
        return False
    mate = mates(lines)
    return all(j is None or (j != i and lines[j][2] == lines[i][1]) for i, j in enumerate(mate))


def closed_form(lines):
    """what a regular file's plan is without the dictionary: a line is the second of a pair iff its mate stands in front of it"""
    plan = []
    for i, j in enumerate(mates(lines)):
        if not lines[i][0]:
            plan.append((i, i))
        elif j is not None and j < i:
            plan += [(j, j), (i, j)]
    return plan


def test_corpus_is_the_goldens():
    assert [c["name"] for c in CASES] == [c["name"] for c in GOLDEN["cases"]]
    for case in CASES:
        assert (EXPECTED[case["name"]]["expected"]["status"] != 0) == (case["error"] is not None), case["name"]
    kinds = {EXPECTED[c["name"]]["expected"]["exception"] for c in CASES if c["error"] is not None}
    assert kinds == {"ValueError", "KeyError", "IndexError", "AttributeError", "UnboundLocalError", None}
    messages = {EXPECTED[c["name"]]["expected"]["stderr"] for c in CASES if c["error"] is not None}
    assert messages == {"", group_multiline.FORMAT_MESSAGE % "XX", group_multiline.COLUMNS_MESSAGE}
    assert {c["n_samples"] for c in CASES} >= {0, 1, 3}
    with open(os.path.join(ROOT, "svtyper_amd", "csrc", "svt_radix_sort_kernel.h")) as f:
        sort = f.read()                                             # the tile of the radix sort, read from its header
    block = int(re.search(r"constexpr int kSortBlock = (\d+);", sort).group(1))
    rounds = int(re.search(r"constexpr uint32_t kSortRounds = (\d+);", sort).group(1))
    assert re.search(r"constexpr uint32_t kSortTile = kSortBlock \* kSortRounds;", sort) and K.SORT_TILE == block * rounds
    pairs = {sum(1 for bnd, _i, _m in read(c) if bnd) // 2 for c in CASES if c["name"].startswith("pairs_")}
    assert pairs >= {1, 2, 63, 64, 65, 257, K.SORT_TILE // 2 + 1}
    most = max((c for c in CASES if c["name"].startswith("pairs_")), key=lambda c: len(c["vcf"]))
    assert K.SORT_TILE < sum(1 for bnd, _i, _m in read(most) if bnd) <= K.SORT_TILE + 2     # one pair more than a tile holds
    only = EXPECTED["unpaired_only"]["expected"]["stdout"]
    assert only.endswith("S0001\n") and only.count("\n#CHROM") == 1               # a header and no body
    first = EXPECTED["mate_takes_the_first_ones_samples"]["expected"]["stdout"].splitlines()[-1].split("\t")
    assert first[2] == "b" and first[5] == "1.00" and first[6] == "LOW" and first[8:] == ["GT:AP", "0/1:4", "1/1:5", "./.:6"]
    assert EXPECTED["samples_0"]["expected"]["stdout"].splitlines()[-1].endswith("\t\t")


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_engine_gives_the_reference_bytes(case, tmp_path):
    golden = EXPECTED[case["name"]]["expected"]
    body = [l for l in case["vcf"].splitlines() if not l.startswith("#")]
    if case["error"] is not None:
        written = io.StringIO()
        stats = {}
        with pytest.raises(group_multiline.GroupError) as e:
            group_multiline.group_multiline(K.write_case(case, str(tmp_path)), vcf_out=written, file_date=GOLDEN["file_date"], stats=stats)
        assert e.value.line == case["error"] and os.path.basename(e.value.file) == "calls.vcf"
        assert written.getvalue() == golden["stdout"]               # the lines in front of the one the script dies on
        assert e.value.reference == golden["exception"]
        assert (e.value.verbatim or "") == golden["stderr"]
        if case["kind"] is not None:
            assert stats["host_lines"] == case["slow_lines"]
            assert [tuple(p) for p in stats["plan"].tolist()] == sequential(read(case))
        return
    text, stats = run(case, tmp_path)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"] and stats["host_join"] is True
    recs = stats["records"]
    assert int((recs["slow"] != 0).sum()) == case["slow_lines"] and stats["lines"] == len(body) == len(recs)
    lines = read(case)
    assert [tuple(p) for p in stats["plan"].tolist()] == sequential(lines) and stats["written"] == len(stats["plan"])
    clean = recs["slow"] == 0
    assert ((recs["flags"][clean] & nr.GROUP_BND != 0) == [l[0] for l, c in zip(lines, clean) if c]).all()
    for rec, raw, (bnd, ident, mate) in zip(recs, body, lines):     # the spans are the ID's and the MATEID value's
        if rec["slow"]:
            continue
        assert raw[rec["id_b"]:rec["id_b"] + rec["id_n"]] == ident
        if bnd and mate is not None:
            assert raw[rec["mate_b"]:rec["mate_b"] + rec["mate_n"]] == mate and rec["flags"] & nr.GROUP_HAS_MATE


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_closed_form_is_the_dictionary_on_the_corpus(case):
    if case["kind"] is None and case["error"] is not None:
        return                                                      # (no #CHROM line: nothing is joined)
    lines = read(case)
    if case["error"] is None:
        assert regular(lines) == (not case["irregular"])
    if regular(lines):
        assert closed_form(lines) == sequential(lines)


def test_closed_form_is_the_dictionary_on_random_small_files():
    """a few thousand files over four IDs: wherever the file is regular the closed form is the script's loop, and the files
    that are not regular are many and differ from it somewhere (so the condition is not vacuous)"""
    rng = random.Random(20240607)
    ids = ["a", "b", "c", "d"]
    n_regular = n_irregular = differs = 0
    for _ in range(6000):
        lines = []
        for _k in range(rng.randrange(1, 8)):
            if rng.random() < 0.2:
                lines.append((False, rng.choice(ids), None))
            else:
                lines.append((True, rng.choice(ids), rng.choice(ids + ["nobody", None])))
        if regular(lines):
            n_regular += 1
            assert closed_form(lines) == sequential(lines), lines
        else:
            n_irregular += 1
            differs += closed_form(lines) != sequential(lines)
    assert n_regular > 500 and n_irregular > 500 and differs > 100


def test_an_error_names_the_key_and_the_token(tmp_path):
    for name, token, word in (("error_no_end_middle", "END", "INFO has no END"), ("error_cipos_no_integer_last", "", "no integer"),
                              ("error_pair_cipos_no_integer_on_the_first_first", "0.5", "0.5"), ("error_bare_ciend_first", "CIEND", "no value")):
        case = next(c for c in CASES if c["name"] == name)
        with pytest.raises(group_multiline.GroupError) as e:
            run(case, tmp_path)
        assert (e.value.token or "") == token and word in str(e.value) and ", line %d" % case["error"] in str(e.value)


def test_gzipped_input_by_name_by_content_and_as_an_open_file(tmp_path):
    case = next(c for c in CASES if c["name"] == "pairs_65")
    vcf = K.write_case(case, str(tmp_path))
    for path in (vcf + ".gz", str(tmp_path / "no_suffix")):
        with open(vcf, "rb") as f, gzip.open(path, "wb") as z:
            z.write(f.read())
    want = EXPECTED["pairs_65"]["expected"]["stdout"]
    for source in (vcf + ".gz", str(tmp_path / "no_suffix")):
        out = io.StringIO()
        group_multiline.group_multiline(source, vcf_out=out, file_date=GOLDEN["file_date"])
        assert out.getvalue() == want
    for path in (vcf, str(tmp_path / "no_suffix")):
        out = io.StringIO()
        with open(path, "rb") as f:                                 # (buffered: it can peek)
            group_multiline.group_multiline(f, vcf_out=out, file_date=GOLDEN["file_date"])
        assert out.getvalue() == want


def test_bcf_input(tmp_path):
    case = K.bcf_case()
    path = str(tmp_path / "calls.bcf")
    out = bcf_out.open_bcf(path)
    out.write(case["vcf"])
    out.close()
    text = bcf_in.open_text(path).read()
    assert len(text.splitlines()) == len(case["vcf"].splitlines())
    want, got, sniffed = io.StringIO(), io.StringIO(), io.StringIO()
    group_multiline.group_multiline(io.BytesIO(text), vcf_out=want, file_date="20240101")
    group_multiline.group_multiline(path, vcf_out=got, file_date="20240101")
    other = str(tmp_path / "no_suffix")
    os.replace(path, other)
    group_multiline.group_multiline(other, vcf_out=sniffed, file_date="20240101")
    assert got.getvalue() == sniffed.getvalue() == want.getvalue()
    assert len([l for l in want.getvalue().splitlines() if "SVTYPE=BND" in l]) == 10


def test_keep_contigs_places_the_lines_before_chrom(tmp_path):
    case = next(c for c in CASES if c["name"] == "pairs_2")
    plain, _s = run(case, tmp_path)
    kept, _s = run(case, tmp_path, keep_contigs=True)
    lines = kept.splitlines()
    at = next(k for k, l in enumerate(lines) if l.startswith("#CHROM"))
    assert lines[at - 1] == "##contig=<ID=1,length=249250621>" and "##contig" not in plain
    assert [l for l in lines if not l.startswith("##contig")] == plain.splitlines()


def command(case, tmp_path, more, stdin=False, module="svtyper_amd.group_multiline", write=K.write_case):
    vcf = write(case, str(tmp_path))
    cmd = [sys.executable, "-m", module] + ([] if stdin else [vcf]) + more
    if stdin:
        with open(vcf, "rb") as f:
            return subprocess.run(cmd, stdin=f, capture_output=True, cwd=ROOT, timeout=120)
    return subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=120)


def dated(text):
    """(the command line has no file_date: the line is the clock's)"""
    return "\n".join(("##fileDate=" + GOLDEN["file_date"]) if l.startswith("##fileDate=") else l for l in text.split("\n"))


@pytest.mark.parametrize("name,stdin", [("unpaired_around_pairs", False), ("chain", True), ("error_undeclared_format_key_middle", False),
                                        ("error_seven_columns_last", True), ("error_pair_cipos_missing_on_the_second_last", False)])
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
    case = next(c for c in CASES if c["name"] == "pairs_65")
    out = str(tmp_path / "grouped.vcf.gz")
    r = command(case, tmp_path, ["--keep-contigs", "--bgzf", "--sort", "--tabix", "-o", out])
    assert r.returncode == 0, r.stderr
    kept, _s = run(case, tmp_path, keep_contigs=True)
    raw = open(out, "rb").read()
    members = X.Members(raw)
    assert dated(members.text().decode()).encode() == X.sorted_text(kept.encode())
    tbi = X.read_tbi(open(out + ".tbi", "rb").read())
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(members.text(), n_random=50), members)

"""Where `classic.sv_genotype` and `singlesample.sso_genotype` differ ON PURPOSE -- the places where the reference's two
programs differ (svtyper/classic.py:107-533 against svtyper/singlesample.py:764-814) and that no other test pins: a
missing VCF, a VCF without a body, `#` lines in the body, sample columns of other tools, a bad alignment path, lines
passed through with their warning, unpaired breakends, `--sum_quals` over an incoming QUAL, `debug`, and `--help`.

CPU only: the likelihood seam is filled by the oracle (as in test_host_pipeline.py); every case runs through the
portable Python reader and through what a caller with the reference's positional arguments gets (`reader=None`: the
C++ reader and the bulk VCF route), on cut-down copies of tests/data/example.vcf of a dozen lines."""
import importlib
import io
import json
import logging
import os
import re
import sys

import pytest

from svtyper_amd import classic, singlesample
from test_host_pipeline import IN_BAM, IN_VCF, LIB_JSON, oracle_engine

HERE = os.path.dirname(os.path.abspath(__file__))
READERS = ["python", None]

with open(IN_VCF) as _f:
    _LINES = _f.readlines()
HEAD = "".join(l for l in _LINES if l.startswith("##"))
CHROM = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
BODY = [l for l in _LINES if not l.startswith("#")]
DELS = BODY[:6]
BND_A, BND_B = (next(l for l in BODY if l.split("\t")[2] == i) for i in ("894054_1", "894054_2"))
SMALL = DELS[:3] + [BND_A] + DELS[3:] + [BND_B]     # a BND pair around three other sites
NO_READS = "2\t1000\tnoreads\tN\t<DEL>\t0\t.\tSVTYPE=DEL;SVLEN=-500;END=1500;CIPOS=-10,10;CIEND=-10,10\n"   # nothing of the fixture BAM lies there


class Sink(io.StringIO):
    def close(self):      # sv_genotype closes its output; the text is still wanted afterwards
        pass


def text_of(body, chrom=CHROM):
    return HEAD + chrom + "".join(body)


def run_classic(text, reader, bam=IN_BAM, lib=LIB_JSON, debug=False, sum_quals=False, num_samp=1000000, **kw):
    out = Sink()
    classic.sv_genotype(bam, None if text is None else io.StringIO(text), out, 20, 1, 1, num_samp, lib, debug, None, None,
                        sum_quals, None, 1e10, engine=oracle_engine, reader=reader, **kw)
    return out.getvalue()


def run_sso(text, reader, bam=IN_BAM, lib=LIB_JSON, debug=False, sum_quals=False, **kw):
    out = Sink()
    singlesample.sso_genotype(bam, None if text is None else io.StringIO(text), out, 20, 1, 1, 1000000, lib, debug, None,
                              sum_quals, 1000, 1e10, None, 1000, engine=oracle_engine, reader=reader, **kw)
    return out.getvalue()


RUN = {"classic": run_classic, "sso": run_sso}


def body_of(text):
    return [l for l in text.split("\n") if l and not l.startswith("#")]


def column_line(text):
    return [l for l in text.split("\n") if l.startswith("#CHROM")]


def no_date(text):
    return [l for l in text.split("\n") if not l.startswith("##fileDate=")]


def no_stamp(err):
    """logit's lines without their `[ 2024-01-31 12:00:00 ]` stamps"""
    return re.sub(r"(?m)^\[ \d{4}-\d\d-\d\d \d\d:\d\d:\d\d \] ", "", err)


# ---------------------------------------------------------------------------------------------- no VCF
@pytest.mark.parametrize("reader", READERS)
def test_classic_without_a_vcf_writes_the_library_file_and_warns(tmp_path, capsys, reader):
    """classic.py:136-180: the BAMs are opened, the libraries computed and written, then the run ends"""
    lib = str(tmp_path / "lib.json")
    assert run_classic(None, reader, lib=lib, num_samp=2000) == ""
    assert capsys.readouterr().err == "Warning: VCF not found.\n"
    with open(lib) as f:
        info = json.load(f)
    assert list(info) == ["NA12878"] and info["NA12878"]["mapped"] == 42801


@pytest.mark.parametrize("reader", READERS)
def test_sso_without_a_vcf_opens_and_writes_nothing(tmp_path, capsys, reader):
    """singlesample.py:780-781 in front of everything else: not even the alignment path is looked at"""
    lib = str(tmp_path / "lib.json")
    assert run_sso(None, reader, bam=str(tmp_path / "not_there.bam"), lib=lib) == ""
    assert not os.path.exists(lib) and os.listdir(str(tmp_path)) == []
    assert capsys.readouterr() == ("", "")


# ---------------------------------------------------------------------------------------------- a header and nothing else
@pytest.mark.parametrize("reader", READERS)
def test_header_only_vcf(reader):
    """classic writes its header when it meets the first body line (classic.py:191-210), so here never; sso always
    writes it (singlesample.py:580), with the BAM's sample as the only column (singlesample.py:112-125)"""
    assert run_classic(text_of([]), reader) == ""
    got = run_sso(text_of([]), reader)
    assert body_of(got) == [] and got.endswith("\n")
    assert got.rstrip("\n").split("\n")[-1] == CHROM.rstrip("\n") + "\tFORMAT\tNA12878"
    assert got.startswith("##fileformat=")


# ---------------------------------------------------------------------------------------------- '#' in the body
@pytest.mark.parametrize("reader", READERS)
def test_sso_skips_hash_lines_in_the_body(reader):
    """singlesample.py's vcf_variants() drops every line that starts with '#', wherever it stands"""
    stats = {}
    plain = run_sso(text_of(SMALL), reader)
    got = run_sso(text_of(SMALL[:2] + ["#a comment\n", "##late=header\n"] + SMALL[2:]), reader, stats=stats)
    assert stats["route"] == ("per line" if reader == "python" else "bulk")
    assert no_date(got) == no_date(plain) and len(body_of(got)) == len(SMALL)


# ---------------------------------------------------------------------------------------------- other tools' sample columns
def test_foreign_sample_column():
    """sso parses only the '##' lines, so the input's samples are not carried over (singlesample.py:112-125); classic keeps
    them and adds the samples the VCF does not name (classic.py:204-207).  Same bytes whichever reader."""
    chrom = CHROM.rstrip("\n") + "\tFORMAT\tOTHER\n"
    body = [l.rstrip("\n") + "\tGT\t0/1\n" for l in SMALL]
    for name, cols in (("sso", ["NA12878"]), ("classic", ["OTHER", "NA12878"])):
        stats = {}
        got = RUN[name](text_of(body, chrom), "python")
        assert no_date(RUN[name](text_of(body, chrom), None, stats=stats)) == no_date(got), name
        assert column_line(got) == [CHROM.rstrip("\n") + "\tFORMAT\t" + "\t".join(cols)], name
        lines = body_of(got)
        assert len(lines) == len(SMALL) and all(len(l.split("\t")) == 9 + len(cols) for l in lines), name
        if name == "classic":
            assert all(l.split("\t")[9].split(":")[0] == "0/1" for l in lines)      # OTHER's genotype is still there
            assert stats["route"] == "per line"       # every line keeps its Genotype objects


def test_sso_notes_a_sample_the_vcf_does_not_name(capsys):
    run_sso(text_of(SMALL), "python")
    assert "Note: Did not find sample name : 'NA12878' in input vcf: '<stdin>' -- adding\n" in no_stamp(capsys.readouterr().err)
    run_sso(text_of(SMALL, CHROM.rstrip("\n") + "\tFORMAT\tNA12878\n"), "python")
    assert "Did not find sample name" not in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------- a bad alignment path
@pytest.mark.parametrize("reader", READERS)
def test_classic_bad_alignment_path(capsys, reader):
    """classic.py:124-132: every name of the comma list, the message on stderr, exit code 1"""
    with pytest.raises(SystemExit) as e:
        run_classic(text_of(SMALL), reader, bam=IN_BAM + ",reads.txt")
    assert e.value.code == 1
    assert capsys.readouterr().err == "Error: reads.txt is not a valid alignment file (*.bam or *.cram)\n"


@pytest.mark.parametrize("reader", READERS)
def test_sso_bad_alignment_path(capsys, reader):
    """singlesample.py:49-51,783: the absolute path, the message as the exit status"""
    with pytest.raises(SystemExit) as e:
        run_sso(text_of(SMALL), reader, bam="reads.txt")
    assert e.value.code == "Error: %s is not a valid alignment file (*.bam or *.cram)\n" % os.path.abspath("reads.txt")
    assert capsys.readouterr() == ("", "")


# ---------------------------------------------------------------------------------------------- lines passed through
NO_SVTYPE = DELS[1].replace("SVTYPE=DEL;", "")
ODD_SVTYPE = DELS[2].replace("SVTYPE=DEL;", "SVTYPE=INS;")
WARNINGS = ("Warning: SVTYPE missing at variant %s. Skipping.\n" % NO_SVTYPE.split("\t")[2]
            + "Warning: Unsupported SVTYPE at variant %s (INS). Skipping.\n" % ODD_SVTYPE.split("\t")[2])


@pytest.mark.parametrize("reader", READERS)
@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_lines_without_a_usable_svtype_pass_through(capsys, driver, reader):
    """classic.py:220-231 warns on stderr as it is; singlesample.py:595-609 through logit (a stamp in front, and print's
    newline behind the message's own)"""
    body = [DELS[0], NO_SVTYPE, ODD_SVTYPE, DELS[3]]
    got = body_of(RUN[driver](text_of(body), reader))
    err = capsys.readouterr().err
    assert [l.split("\t")[:5] for l in got] == [l.split("\t")[:5] for l in body]
    for line, src in list(zip(got, body))[1:3]:
        cols = line.split("\t")
        assert cols[5] == "0.00" and cols[8:] == ["GT", "./."], line
        assert ("SVTYPE" in cols[7]) == ("SVTYPE" in src)
    assert got[0].split("\t")[9].split(":")[0] in ("0/0", "0/1", "1/1")
    if driver == "classic":
        assert err == WARNINGS
    else:
        stamped = [l for l in err.split("\n") if "Warning" in l]
        assert len(stamped) == 2 and all(re.match(r"^\[ \d{4}-\d\d-\d\d \d\d:\d\d:\d\d \] Warning", l) for l in stamped)
        assert WARNINGS.replace("\n", "\n\n") in no_stamp(err)


def test_passed_through_lines_are_the_same_bytes_on_both_routes():
    body = [DELS[0], NO_SVTYPE, ODD_SVTYPE, DELS[3]]
    for driver in ("classic", "sso"):
        assert no_date(RUN[driver](text_of(body), "python")) == no_date(RUN[driver](text_of(body), None)), driver


# ---------------------------------------------------------------------------------------------- unpaired breakends
@pytest.mark.parametrize("reader", READERS)
def test_classic_warns_about_unpaired_breakends(caplog, reader):
    """the first mate waits for a partner that never comes: classic says so and both drivers leave the line out"""
    with caplog.at_level(logging.WARNING):
        got = body_of(run_classic(text_of(DELS[:3] + [BND_A] + DELS[3:]), reader))
    assert [r.getMessage() for r in caplog.records] == ["Unpaired breakends found in file. These will not be present in output."]
    assert [l.split("\t")[2] for l in got] == [l.split("\t")[2] for l in DELS]


@pytest.mark.parametrize("reader", READERS)
def test_sso_drops_unpaired_breakends_silently(caplog, capsys, reader):
    with caplog.at_level(logging.WARNING):
        got = body_of(run_sso(text_of(DELS[:3] + [BND_A] + DELS[3:]), reader))
    assert caplog.records == [] and "npaired" not in capsys.readouterr().err
    assert [l.split("\t")[2] for l in got] == [l.split("\t")[2] for l in DELS]


# ---------------------------------------------------------------------------------------------- --sum_quals
def with_qual(line, qual):
    cols = line.split("\t")
    cols[5] = qual
    return "\t".join(cols)


@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_sum_quals_over_an_incoming_qual(driver):
    """QUAL in + SQ of every called sample (classic.py:485, singlesample.py:544-546); a sample without evidence resets
    classic's QUAL (classic.py:496-498) and leaves sso's alone; the second BND mate is written with the first one's"""
    body = [with_qual(l, "12.5") for l in SMALL + [NO_READS]]
    plain = body_of(RUN[driver](text_of(body), "python"))
    summed = body_of(RUN[driver](text_of(body), "python", sum_quals=True))
    assert no_date(RUN[driver](text_of(body), None, sum_quals=True)) == no_date(RUN[driver](text_of(body), "python", sum_quals=True))
    assert len(plain) == len(summed) == len(body)
    for a, b in zip(plain, summed):
        a, b = a.split("\t"), b.split("\t")
        assert a[:5] + a[6:] == b[:5] + b[6:]
        if a[2] == "noreads":
            assert a[9].startswith("./.") and a[5] == "0.00" and b[5] == ("0.00" if driver == "classic" else "12.50")
        else:
            assert a[9].split(":")[0] in ("0/0", "0/1", "1/1")
            assert abs(float(b[5]) - float(a[5]) - 12.5) < 0.011       # two numbers printed with %0.2f
    mates = [l.split("\t") for l in summed if l.split("\t")[2].startswith("894054_")]
    assert len(mates) == 2 and mates[0][5] == mates[1][5] and float(mates[0][5]) > 12.5


# ---------------------------------------------------------------------------------------------- debug
@pytest.mark.parametrize("reader", READERS)
def test_classic_debug_prints_the_tallies_and_keeps_to_the_per_line_route(capsys, reader):
    """classic.py:410-419 prints five tallies and the likelihoods of every (site, sample) on stdout; the bulk route
    has no such print, so debug keeps every line on the per-line route"""
    stats = {}
    quiet = run_classic(text_of(SMALL), reader)
    capsys.readouterr()
    got = run_classic(text_of(SMALL), reader, debug=True, stats=stats)
    out = capsys.readouterr().out.split("\n")
    assert stats["route"] == "per line"
    assert no_date(got) == no_date(quiet)
    n_sites = len(SMALL) - 1
    assert out.count("--------------------------") == n_sites
    blocks = "\n".join(out).split("--------------------------\n")[1:]
    for block in blocks:
        lines = block.rstrip("\n").split("\n")
        assert [l.split(":")[0] for l in lines[:5]] == ["ref_span", "alt_span", "ref_seq", "alt_seq", "alt_clip"]
        assert len(lines) == 6 and re.match(r"^\[-?[\d.e+-]+, -?[\d.e+-]+, -?[\d.e+-]+\]$", lines[5]), lines
    if reader is None:      # the same numbers whichever reader collected the evidence
        run_classic(text_of(SMALL), "python", debug=True)
        assert capsys.readouterr().out.split("\n") == out


@pytest.mark.parametrize("reader", READERS)
def test_sso_debug_changes_neither_route_nor_stderr(capsys, reader):
    """sso_genotype's own debug lines belong to the seams (tally_variant_read_fragments, bayesian_genotype); the driver logs
    the same lines with and without it, and does not leave the bulk route"""
    quiet = run_sso(text_of(SMALL), reader)
    err_quiet = no_stamp(capsys.readouterr().err)
    stats = {}
    got = run_sso(text_of(SMALL), reader, debug=True, stats=stats)
    cap = capsys.readouterr()
    assert stats["route"] == ("per line" if reader == "python" else "bulk")
    assert no_date(got) == no_date(quiet)
    assert cap.out == "" and no_stamp(cap.err) == err_quiet
    assert "Genotyping Input VCF (Serial Mode)\n" in err_quiet


# ---------------------------------------------------------------------------------------------- --help
@pytest.mark.parametrize("module,prog", [(classic, "svtyper"), (singlesample, "svtyper-sso")])
def test_help_text(monkeypatch, capsys, module, prog):
    """`--help` of both programs, byte for byte (tests/golden/help_<prog>.txt, 80 columns)"""
    monkeypatch.setenv("COLUMNS", "80")
    monkeypatch.setattr(sys, "argv", [prog, "--help"])
    with pytest.raises(SystemExit) as e:
        module.get_args()
    assert e.value.code == 0
    with open(os.path.join(HERE, "golden", "help_%s.txt" % prog)) as f:
        assert capsys.readouterr().out == f.read()


@pytest.mark.parametrize("prog", ["classify", "update_info", "group_multiline", "paste", "bcf_in"])
def test_cohort_help_text(monkeypatch, capsys, prog):
    """`--help` of the cohort programs, byte for byte (tests/golden/help_<prog>.txt, 80 columns): the options they share are added
    by one function (cohort.add_program_arguments), behind each program's own"""
    monkeypatch.setenv("COLUMNS", "80")
    with pytest.raises(SystemExit) as e:
        importlib.import_module("svtyper_amd." + prog).get_args(["--help"])
    assert e.value.code == 0
    with open(os.path.join(HERE, "golden", "help_%s.txt" % prog)) as f:
        assert capsys.readouterr().out == f.read()

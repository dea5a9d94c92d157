"""BCF as an input of the programs (svtyper_amd/bcf_in.py; cohort.open_source; driver.gzip_text), on the host: update_info, classify
and paste over their golden cases that a BCF can hold, the input first written through the BCF writer, give the output of the same
case fed the decoded text; sso_genotype with -i as a BCF gives the bytes it gives for the decoded VCF; is_bcf; BcfInputError with
file, record and kind; the bcf_in command line on a valid file, into a sorted indexed .vcf.gz, and on bad files.  No GPU."""
import gzip
import io
import os
import subprocess
import sys

import pytest

import bcftextcases as C
import classifycases as KC
import pastecases as P
import test_classify_host as HC
import test_host_pipeline as T
import test_paste_host as HP
import test_update_info_host as HU
import updateinfocases as KU

from svtyper_amd import bcf_in, bcf_out, classify, driver, hip, paste, singlesample, update_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_bcf(path, text):
    """`text` through the BCF writer: True, or False where a BCF cannot hold it (an undeclared contig or key)"""
    out = bcf_out.open_bcf(path)
    out.write(text)
    try:
        out.close()
    except (bcf_out.BcfError, hip.SvtyperHipError):      # (a record the header does not cover; a text without #CHROM line)
        return False
    return True


def decoded(path):
    return bcf_in.open_text(path).read()


def holdable(cases, tmp_path, key="vcf"):
    """[(case, the path of its input as a BCF)] for the cases without an error whose input a BCF holds"""
    out = []
    for case in cases:
        path = str(tmp_path / (case["name"] + ".bcf"))
        if case.get("error") is None and write_bcf(path, case[key]):
            out.append((case, path))
    return out


def test_update_info_reads_bcf(tmp_path):
    held = holdable(HU.CASES + [KU.bcf_case()], tmp_path)
    assert len(held) >= 20 and any(c["n_samples"] >= 65 for c, _ in held)
    for case, path in held:
        want, got, sniffed = io.StringIO(), io.StringIO(), io.StringIO()
        text = decoded(path)
        assert len(text.splitlines()) == len(case["vcf"].splitlines())
        update_info.update_info(io.BytesIO(text), vcf_out=want, file_date="20240101")
        update_info.update_info(path, vcf_out=got, file_date="20240101")
        assert got.getvalue() == want.getvalue(), case["name"]
        other = str(tmp_path / "no_suffix")
        os.replace(path, other)
        with open(other, "rb") as f:                # by content: a path without the suffix, and an open file
            update_info.update_info(f, vcf_out=sniffed, file_date="20240101")
        assert sniffed.getvalue() == want.getvalue()
        sniffed = io.StringIO()
        update_info.update_info(other, vcf_out=sniffed, file_date="20240101")
        assert sniffed.getvalue() == want.getvalue()


def test_classify_reads_bcf(tmp_path):
    cases = [c for c in HC.CASES + [KC.bcf_case()] if c.get("error") is None]
    done = 0
    for case in cases:
        path = str(tmp_path / (case["name"] + ".bcf"))
        if not write_bcf(path, with_contigs(case["vcf"])):
            continue
        _vcf, gender, exclude, annotation = KC.write_case(case, str(tmp_path))
        text = decoded(path)
        want, got = io.StringIO(), io.StringIO()
        classify.classify(io.BytesIO(text), gender, exclude, annotation, vcf_out=want, file_date="20240101", **case["options"])
        classify.classify(path, gender, exclude, annotation, vcf_out=got, file_date="20240101", **case["options"])
        assert got.getvalue() == want.getvalue(), case["name"]
        done += bool(want.getvalue())
    assert done >= 20


def holdable_input(text, master):
    """a paste input as a genotyper writes it, so that a BCF holds it: the goldens' inputs behind the first carry a bare header, and
    none declares its contigs or the body's EVENT -- each gets the master's declarations, EVENT's and the ##contig lines"""
    lines = text.splitlines(True)
    if not any(l.startswith("##INFO=") for l in lines):
        lines[1:1] = [l for l in master.splitlines(True) if l.startswith(("##INFO=", "##FORMAT=", "##ALT=", "##FILTER="))]
    if not any(l.startswith("##INFO=<ID=%s," % P.DROPPED_INFO) for l in lines):
        lines[1:1] = ['##INFO=<ID=%s,Number=1,Type=String,Description="ID of event">\n' % P.DROPPED_INFO]
    return with_contigs("".join(lines))


def test_paste_reads_a_list_of_bcf(tmp_path):
    done = 0
    for case in HP.CASES:
        if case.get("error") is not None:
            continue
        master, paths = P.write_case(case, str(tmp_path))
        packed, texts = [], []
        for k, text in enumerate(case["inputs"]):
            packed.append(str(tmp_path / ("in%03d.bcf" % k)))
            if not write_bcf(packed[-1], holdable_input(text, case["master"] or case["inputs"][0])):
                break
            texts.append(str(tmp_path / ("dec%03d.vcf" % k)))
            with open(texts[-1], "wb") as f:
                f.write(decoded(packed[-1]))
        else:
            want, got = io.StringIO(), io.StringIO()
            paste.paste(texts, master=master, vcf_out=want, file_date="20240101", **P.case_options(case))
            paste.paste(packed, master=master, vcf_out=got, file_date="20240101", **P.case_options(case))
            assert got.getvalue() == want.getvalue(), case["name"]
            done += bool(want.getvalue())
    assert done >= 10


def with_contigs(text):
    """`text` with a ##contig line for every CHROM of its body that it does not declare, so that a BCF holds it"""
    lines = text.splitlines(True)
    at = next((k for k, l in enumerate(lines) if l.startswith("#CHROM")), None)
    if at is None:
        return text
    declared = [l[len("##contig=<ID="):].split(",")[0].rstrip(">\n") for l in lines[:at] if l.startswith("##contig=<ID=")]
    contigs = []
    for l in lines[at + 1:]:
        if l.split("\t")[0] not in contigs + declared:
            contigs.append(l.split("\t")[0])
    return "".join(lines[:at] + ["##contig=<ID=%s,length=250000000>\n" % c for c in contigs] + lines[at:])


def test_sso_genotype_reads_sites_from_a_bcf(tmp_path):
    path = str(tmp_path / "sites.bcf")
    with open(T.IN_VCF) as f:
        assert write_bcf(path, with_contigs(f.read()))
    text = decoded(path).decode()
    assert bcf_in.is_bcf(path) and text.count("\n") > 200

    def run(vcf_in):
        sink = io.StringIO()
        singlesample.sso_genotype(T.IN_BAM, vcf_in, sink, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                  engine=T.oracle_engine, reader="python")
        return [l for l in sink.getvalue().split("\n") if not l.startswith("##fileDate=")]

    handle = open(path)
    vcf_in = driver.gzip_text(handle)
    assert vcf_in is not handle and handle.closed
    assert run(vcf_in) == run(io.StringIO(text))


def test_is_bcf(tmp_path):
    stream, _want = C.idx_stream()
    bcf, gz, plain = str(tmp_path / "a"), str(tmp_path / "b.gz"), str(tmp_path / "c.vcf")
    assert write_bcf(bcf, KU.bcf_case()["vcf"])
    with gzip.open(gz, "wb") as f:
        f.write(b"BCF\2\2 is what a gzip of text may begin with")
    with open(plain, "wb") as f:
        f.write(stream)
    assert bcf_in.is_bcf(bcf) and not bcf_in.is_bcf(gz) and not bcf_in.is_bcf(plain)
    with open(bcf, "rb") as f:
        assert bcf_in.is_bcf(f) and f.tell() == 0
    assert not bcf_in.is_bcf(io.BytesIO(b"BCF\2\2"))


class _Kept(io.BytesIO):
    def close(self):                                # (the writer closes its sink: the bytes are read afterwards)
        pass


def bgzf_of(stream):
    from svtyper_amd import bam
    sink = _Kept()
    w = bam.BgzfWriter(sink)
    w.write(stream)
    w.close()
    return sink.getvalue()


def test_errors_name_the_file_the_record_and_the_kind(tmp_path):
    refused = {r[0]: r for r in C.refusals()}
    for name in ("gt_as_characters", "contig_in_a_hole", "shared_part_with_a_tail"):
        path = str(tmp_path / (name + ".bcf"))
        with open(path, "wb") as f:
            f.write(bgzf_of(C.refusal_stream(refused[name][2])))
        with pytest.raises(bcf_in.BcfInputError) as e:
            bcf_in.open_text(path)
        assert (e.value.file, e.value.record, e.value.kind) == (path, 2, refused[name][1]) and path in str(e.value) and "record 2" in str(e.value)
        assert isinstance(e.value, ValueError)
    good = bgzf_of(C.idx_stream()[0])
    for name, data, kind in (("cut.bcf", good[:-40], "bgzf"), ("crc.bcf", good[:60] + bytes([good[60] ^ 1]) + good[61:], "bgzf"),
                             ("text.bcf", bgzf_of(b"##fileformat=VCFv4.2\n"), "header"), ("empty.bcf", b"", "bgzf")):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(bcf_in.BcfInputError) as e:
            bcf_in.open_text(path)
        assert e.value.kind == kind and e.value.record is None and e.value.file == path, name


def test_stats_and_chunks(tmp_path):
    path = str(tmp_path / "idx.bcf")
    stream, want = C.idx_stream()
    with open(path, "wb") as f:
        f.write(bgzf_of(stream))
    stats = {}
    f = bcf_in.open_text(path, block_bytes=1, stats=stats)
    assert list(f) == want.encode().splitlines(True) and f.name == path
    assert stats == dict(records=4, chunks=4, host_lines=0, times={})
    with pytest.raises(ValueError):
        bcf_in.open_text(path, engine="gpu")


def test_command_line(tmp_path):
    path, out = str(tmp_path / "idx.bcf"), str(tmp_path / "out.vcf")
    stream, want = C.idx_stream()
    with open(path, "wb") as f:
        f.write(bgzf_of(stream))
    r = subprocess.run([sys.executable, "-m", "svtyper_amd.bcf_in", path, "-o", out], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stderr == "" and open(out).read() == want
    r = subprocess.run([sys.executable, "-m", "svtyper_amd.bcf_in", path], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and r.stdout == want
    packed = str(tmp_path / "x.vcf.gz")
    r = subprocess.run([sys.executable, "-m", "svtyper_amd.bcf_in", path, "--bgzf", "--sort", "--tabix", "-o", packed], capture_output=True, text=True,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    body = [l for l in want.splitlines(True) if not l.startswith("#")]
    order = sorted(range(len(body)), key=lambda k: (("chrB", "chrA").index(body[k].split("\t")[0]), int(body[k].split("\t")[1]), k))
    assert gzip.open(packed, "rt").read() == C.IDX_PRINTED + "".join(body[k] for k in order) and os.path.getsize(packed + ".tbi") > 28
    bad = str(tmp_path / "bad.bcf")
    with open(bad, "wb") as f:
        f.write(bgzf_of(C.refusal_stream(C.refusals()[-1][2])))
    for arg, words in ((bad, "record 2"), (str(tmp_path / "none.bcf"), "No such file")):
        r = subprocess.run([sys.executable, "-m", "svtyper_amd.bcf_in", arg, "-o", out], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith("Error: ") and words in r.stderr, r.stderr

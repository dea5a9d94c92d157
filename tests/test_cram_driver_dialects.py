"""The drivers' words for a CRAM input: the usage errors of pipeline.check_cram through sv_genotype, sso_genotype, the command
line and the sharded run (in front of its first collective), and open_alignment_file's choice of reader without pysam."""
import io
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramcases as cc  # noqa: E402
import cramwriter as cw  # noqa: E402
from svtyper_amd import bam, classic, cram, pipeline, sharded, singlesample  # noqa: E402

VCF = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def sv(bam_string, **kw):
    return classic.sv_genotype(bam_string, io.StringIO(VCF), io.StringIO(), 20, 1, 1, 1000000, None, False, None, None, False, None, 1e10, **kw)


def sso(bam_string, **kw):
    return singlesample.sso_genotype(bam_string, io.StringIO(VCF), io.StringIO(), 20, 1, 1, 1000000, None, False, None, False, 1000, 1e10, None, 1000, **kw)


@pytest.mark.parametrize("call", [sv, sso], ids=["sv_genotype", "sso_genotype"])
@pytest.mark.parametrize("kw", [dict(reader="native"), dict(reader="device"), dict(reader="device", inflate="device"),
                                dict(reader="native", library_scan="device"), dict(inflate="device"), dict(library_scan="device")],
                         ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()))
def test_routes_a_cram_does_not_take(call, kw):
    with pytest.raises(ValueError, match="CRAM input takes the Python reader route"):
        call("/nowhere/sample.cram", **kw)
    if call is sv:
        with pytest.raises(ValueError, match="CRAM input takes the Python reader route"):
            call("/nowhere/a.bam,/nowhere/b.cram", **kw)


@pytest.mark.parametrize("call", [sv, sso], ids=["sv_genotype", "sso_genotype"])
def test_cram_codec_without_a_cram(call):
    with pytest.raises(ValueError, match="cram_codec .* no .cram among the alignment files"):
        call("/nowhere/sample.bam", cram_codec="device")
    with pytest.raises(ValueError, match="cram_codec must be"):
        call("/nowhere/sample.cram", cram_codec="gpu")


def test_check_cram_chooses_the_python_reader():
    assert pipeline.check_cram("a.cram", None) == "python" and pipeline.check_cram("a.bam,b.cram", None, cram_codec="device") == "python"
    assert pipeline.check_cram("a.cram", "python") == "python"
    assert pipeline.check_cram("a.bam", None) is None and pipeline.check_cram("a.bam", "device", "device", "device") == "device"


def test_sharded_runs_refuse_before_their_first_collective():
    # (no process group exists here: a collective would raise something else)
    for run in (sharded.sv_genotype_sharded, sharded.sso_genotype_sharded):
        with pytest.raises(ValueError, match="CRAM input takes the Python reader route"):
            run("/nowhere/s.cram", io.StringIO(VCF), io.StringIO(), 20, 1, 1, 1000000, None, False, None, None, False, None, 1e10,
                rank=1, world=2, reader="device")
        with pytest.raises(ValueError, match="no .cram among"):
            run("/nowhere/s.bam", io.StringIO(VCF), io.StringIO(), 20, 1, 1, 1000000, None, False, None, None, False, None, 1e10,
                rank=1, world=2, cram_codec="host")


@pytest.mark.parametrize("module", [classic, singlesample], ids=["svtyper", "svtyper-sso"])
@pytest.mark.parametrize("argv,says", [(["-B", "s.cram", "--reader", "native"], "Python reader route"),
                                       (["-B", "s.cram", "--library-scan", "device"], "Python reader route"),
                                       (["-B", "s.bam", "--cram-codec", "device"], "no .cram among")])
def test_command_line_usage_errors(module, argv, says, monkeypatch, capsys):
    monkeypatch.setattr(sys, "argv", ["prog"] + argv)
    with pytest.raises(SystemExit) as e:
        module.get_args()
    assert e.value.code == 2 and says in capsys.readouterr().err


def test_open_alignment_file_without_pysam(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "pysam", None)          # (import pysam -> ImportError)
    path = str(tmp_path / "s.cram")
    cw.write_cram(path, cc.HEADER, cc.mixed_records(), cw.Layout())
    f = bam.open_alignment_file(path)
    assert isinstance(f, cram.CramFile) and f.codec == "host" and not f.verify
    assert f.count("chr2", 0, 5000) > 0
    f.close()
    g = bam.open_alignment_file(path, verify=True, cram_codec="device", device=0)
    assert isinstance(g, cram.CramFile) and g.verify and g.codec == "device"
    g.close()
    assert isinstance(bam.open_alignment_file(cc.FIXTURE_BAM), bam.AlignmentFile)
    with pytest.raises(NotImplementedError):
        bam.AlignmentFile(path)

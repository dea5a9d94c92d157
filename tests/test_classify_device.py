"""GPU: svtyper_amd.classify with engine="device" (svtyper_amd/csrc/svt_vcf_classify_kernel.h) over the corpus of
tests/classifycases.py: the golden bytes of the reference's script, the per-line records of the host twin byte for byte (medians,
MADs, slopes and r2 included), the number of lines that left the device (exactly the lines the corpus built for the host's plain
C++: a device path that hands everything to the host does not pass), blocks, and the command line into a sorted, CSI-indexed BCF
file compressed on the device, read back by the independent readers of tests/bcfreader.py and tests/csioutcases.py."""
import io
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import classifycases as K
import test_bcf_host as B
import test_classify_host as H
import test_cohort_line_host as L
from svtyper_amd import classify

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", H.CASES, ids=[c["name"] for c in H.CASES])
def test_device_engine_gives_the_reference_bytes_and_the_hosts_records(case, tmp_path, hip_device):
    golden = H.EXPECTED[case["name"]]["expected"]
    if case["error"] is not None:
        with pytest.raises(classify.ClassifyError) as on_host:
            H.run(case, tmp_path)
        written = io.StringIO()
        with pytest.raises(classify.ClassifyError) as e:
            H.run(case, tmp_path, sink=written, engine="device", device=hip_device)
        assert written.getvalue() == golden["stdout"]               # the lines in front of the one the script dies on
        assert (e.value.line, e.value.reference, e.value.verbatim, str(e.value)) == (on_host.value.line, on_host.value.reference,
                                                                                      on_host.value.verbatim, str(on_host.value))
        return
    _text, host = H.run(case, tmp_path)
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"]
    assert stats["lines"] == host["lines"] and stats["blocks"] == host["blocks"]
    assert H.records(stats).tobytes() == H.records(host).tobytes()
    if stats["blocks"]:
        assert stats["times"]["classify_kernel_s"] > 0


def test_a_regression_on_its_threshold_is_flagged_near_on_the_device(tmp_path, hip_device):
    _text, host = H.run(K.near_case(), tmp_path)
    _text, stats = H.run(K.near_case(), tmp_path, engine="device", device=hip_device)
    assert stats["near_lines"] == 1 and H.records(stats).tobytes() == H.records(host).tobytes()


@pytest.mark.parametrize("name", ["width_65", "width_257", "annotation", "last_line_verbatim_bare"])
def test_three_blocks_on_the_device(name, tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == name)
    body = [l for l in case["vcf"].splitlines(True) if not l.startswith("#")]
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device, block_bytes=sum(map(len, body)) // 3 + 1)
    assert stats["blocks"] >= 3 and text == H.EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]


def test_command_line_to_a_sorted_indexed_bcf_file(tmp_path, hip_device):
    """N = 65: --engine device --bcf --sort --csi --deflate device, in a child process"""
    case = K.bcf_case()
    vcf, gender, _exclude, _annotation = K.write_case(case, str(tmp_path))
    out = str(tmp_path / "classified.bcf")
    cmd = [sys.executable, "-m", "svtyper_amd.classify", "-i", vcf, "-g", gender, "--keep-contigs", "--engine", "device", "--device", str(hip_device),
           "--bcf", "--sort", "--csi", "--deflate", "device", "-o", out]
    date = time.strftime("%Y%m%d")                  # (the command line has no file_date: the line is the clock's)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    want = io.StringIO()
    classify.classify(vcf, gender, vcf_out=want, file_date=date, keep_contigs=True)
    text = want.getvalue()
    assert text.count("SVTYPE=BND") == 4 and text.count("\n1\t") == 7
    assert B.check_indexed(out, text, 1, 249250621)


@pytest.mark.parametrize("k", range(len(L.K.LENGTHS) + len(L.EDGES)))
def test_column_starts_at_every_residue_and_length_on_the_device(k, hip_device):
    """tests/cohortlinecases.py: the sample region at the 16 residues of its address, around one piece, one step and two steps of
    the 128-bit scan, first and last in its block: the host's records and text, and no line leaves the device.  Behind them the
    edges of a call (test_cohort_line_host.EDGES: no text, one line without its newline, two lines): the host's records, reports
    and text there too"""
    records, report, out, wrote = L.host("classify", k)
    got, info, text, written = L.run("classify", (L.blocks("classify") + L.edges("classify"))[k], device=hip_device)
    assert info["host_lines"] == 0 and info["bad_line"] == 0 and written["bad_line"] == 0
    assert got.tobytes() == records.tobytes() and text == out and info == report and written == wrote
    assert len(got) == (16, 0, 1, 2)[max(k - len(L.K.LENGTHS) + 1, 0)]

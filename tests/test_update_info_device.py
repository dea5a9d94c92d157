"""GPU: svtyper_amd.update_info with engine="device" (svtyper_amd/csrc/svt_vcf_update_info_kernel.h) over the corpus of
tests/updateinfocases.py: the golden bytes of the reference's script, the per-line records of the host twin byte for byte (the bits
of sum_sq included: the kernel adds SQ in sample order), the number of lines that left the device (exactly the lines the corpus
built for the host's plain C++: a device path that hands lines to the host does not pass), blocks, and the command line into a
sorted, CSI-indexed BCF file compressed on the device, read back by the independent readers of tests/bcfreader.py and
tests/csioutcases.py."""
import io
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import test_bcf_host as B
import test_cohort_line_host as L
import test_update_info_host as H
import updateinfocases as K
from svtyper_amd import native_reads as nr
from svtyper_amd import update_info

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", H.CASES, ids=[c["name"] for c in H.CASES])
def test_device_engine_gives_the_reference_bytes_and_the_hosts_records(case, tmp_path, hip_device):
    golden = H.EXPECTED[case["name"]]["expected"]
    if case["error"] is not None:
        with pytest.raises(update_info.UpdateInfoError) as on_host:
            H.run(case, tmp_path)
        written = io.StringIO()
        with pytest.raises(update_info.UpdateInfoError) as e:
            H.run(case, tmp_path, sink=written, engine="device", device=hip_device)
        assert written.getvalue() == golden["stdout"]               # the lines in front of the one the script dies on
        assert (e.value.line, e.value.reference, e.value.verbatim, str(e.value)) == (on_host.value.line, on_host.value.reference,
                                                                                      on_host.value.verbatim, str(on_host.value))
        return
    _text, host = H.run(case, tmp_path)
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"]                # exactly: nothing else leaves the device
    assert stats["lines"] == host["lines"] and stats["blocks"] == host["blocks"]
    assert H.records(stats).tobytes() == H.records(host).tobytes()
    if stats["blocks"]:
        assert stats["times"]["update_info_kernel_s"] > 0


def test_only_the_line_wider_than_the_capacity_leaves_the_device(tmp_path, hip_device):
    """4 096 samples stay on the device, 4 097 are the host's: every line of that case and no line of any other width"""
    for case in (c for c in H.CASES if c["name"].startswith("width_") and c["n_samples"]):
        _text, stats = H.run(case, tmp_path, engine="device", device=hip_device)
        flags = H.records(stats)["flags"]
        if case["n_samples"] > K.CAPACITY:
            assert stats["host_lines"] == stats["lines"] == 2 and (flags == nr.UPDATE_INFO_SLOW_CAPACITY).all()
        else:
            assert stats["host_lines"] == 0 and not flags.any()


def test_the_sum_of_sq_is_taken_in_sample_order_on_the_device(tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == "msq_order_matters")
    _text, stats = H.run(case, tmp_path, engine="device", device=hip_device)
    body = [l for l in case["vcf"].splitlines() if not l.startswith("#")]
    for rec, line in zip(H.records(stats), body):
        in_order = sum(H.sq_of(line), 0.0)
        assert rec["flags"] == 0 and rec["sum_sq"] == np.float64(in_order).view(np.uint64) and in_order != H.strided(H.sq_of(line))


@pytest.mark.parametrize("name", ["width_65", "width_257", "format_short_sample_columns", "last_line_bare"])
def test_three_blocks_on_the_device(name, tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == name)
    body = [l for l in case["vcf"].splitlines(True) if not l.startswith("#")]
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device, block_bytes=sum(map(len, body)) // 3 + 1)
    assert stats["blocks"] >= min(3, len(body)) and text == H.EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]


def test_command_line_to_a_sorted_indexed_bcf_file(tmp_path, hip_device):
    """N = 65: --engine device --bcf --sort --csi --deflate device --keep-contigs, in a child process"""
    case = K.bcf_case()
    vcf = K.write_case(case, str(tmp_path))
    out = str(tmp_path / "updated.bcf")
    cmd = [sys.executable, "-m", "svtyper_amd.update_info", vcf, "--keep-contigs", "--engine", "device", "--device", str(hip_device),
           "--bcf", "--sort", "--csi", "--deflate", "device", "-o", out]
    date = time.strftime("%Y%m%d")                  # (the command line has no file_date: the line is the clock's)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    want = io.StringIO()
    update_info.update_info(vcf, vcf_out=want, file_date=date, keep_contigs=True)
    text = want.getvalue()
    assert text.count("\n1\t") == 5 and text.count(";MSQ=") == 5 and "SNAME" not in text
    assert B.check_indexed(out, text, 1, 249250621)


@pytest.mark.parametrize("k", range(len(L.K.LENGTHS) + len(L.EDGES)))
def test_column_starts_at_every_residue_and_length_on_the_device(k, hip_device):
    """tests/cohortlinecases.py: the sample region at the 16 residues of its address, around one piece, one step and two steps of
    the 128-bit scan, first and last in its block: the host's records and text, and no line leaves the device.  Behind them the
    edges of a call (test_cohort_line_host.EDGES: no text, one line without its newline, two lines): the host's records, reports
    and text there too"""
    records, report, out, wrote = L.host("update_info", k)
    got, info, text, written = L.run("update_info", (L.blocks("update_info") + L.edges("update_info"))[k], device=hip_device)
    assert info["host_lines"] == 0 and info["bad_line"] == 0 and written["bad_line"] == 0
    assert got.tobytes() == records.tobytes() and text == out and info == report and written == wrote
    assert len(got) == (16, 0, 1, 2)[max(k - len(L.K.LENGTHS) + 1, 0)]

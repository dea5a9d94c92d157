"""GPU: svtyper_amd.paste with engine="device" (svtyper_amd/csrc/svt_vcf_paste_kernel.h) over the corpus of tests/pastecases.py:
the golden bytes of the reference's scripts, the per-line results of the host twin, the number of lines that left the device
(exactly the lines the corpus built for the slow path: a device path that hands everything to the host does not pass), the
three copy layouts of the write kernel, blocks, `safe`, and the command line into a sorted, tabix-indexed BGZF file compressed on
the device, read back by the independent readers of tests/tbxcases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pastecases as P
import tbxcases as X
import test_paste_host as H
from svtyper_amd import native_reads as nr
from svtyper_amd import paste

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", H.CASES, ids=[c["name"] for c in H.CASES])
def test_device_engine_gives_the_reference_bytes_and_the_hosts_results(case, tmp_path, hip_device):
    golden = H.EXPECTED[case["name"]]["expected"]
    if case["error"] is not None:
        with pytest.raises(paste.PasteError) as on_host:
            H.run(case, tmp_path)
        with pytest.raises(paste.PasteError) as e:
            H.run(case, tmp_path, engine="device", device=hip_device)
        assert (e.value.file, e.value.line, e.value.field, e.value.verbatim) == (on_host.value.file, on_host.value.line, on_host.value.field,
                                                                                 on_host.value.verbatim)
        assert str(e.value) == str(on_host.value)
        return
    _text, host, _m, _p = H.run(case, tmp_path)
    text, stats, _m, _p = H.run(case, tmp_path, engine="device", device=hip_device)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"]
    assert stats["lines"] == host["lines"] and stats["blocks"] == 1
    assert np.concatenate(stats["results"]).tobytes() == np.concatenate(host["results"]).tobytes()
    assert stats["times"]["measure_kernel_s"] > 0 and stats["times"]["write_kernel_s"] > 0


@pytest.mark.parametrize("layout", ["lane", "quarter", "wave"])
@pytest.mark.parametrize("name", ["n3_afreq_shapes", "n65_slow_second_stride", "n130_afreq_q_m"])
def test_every_copy_layout_writes_the_same_bytes(name, layout, tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == name)
    text, _stats, _m, _p = H.run(case, tmp_path, engine="device", device=hip_device, layout=layout)
    assert text == H.EXPECTED[name]["expected"]["stdout"]


@pytest.mark.parametrize("name", ["n3_afreq_shapes_q", "n65_slow_second_stride", "n130_plain_q"])
def test_three_blocks_on_the_device(name, tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == name)
    row = sum(len(t.splitlines()[-1]) + 1 for t in case["inputs"]) + 400
    text, stats, _m, _p = H.run(case, tmp_path, engine="device", device=hip_device, block_bytes=2 * row)
    assert stats["blocks"] >= 3 and text == H.EXPECTED[name]["expected"]["stdout"]
    assert stats["host_lines"] == case["slow_lines"]


def test_safe_on_the_device(tmp_path, hip_device):
    case = H.unsafe_case()
    for block_bytes in (None, 4000):
        with pytest.raises(paste.PasteError) as e:
            H.run(case, tmp_path, engine="device", device=hip_device, safe=True, block_bytes=block_bytes)
        assert (os.path.basename(e.value.file), e.value.line, e.value.field) == ("in001.vcf", 2 + 18, "POS")
    whole = next(c for c in H.CASES if c["name"] == "n3_forty_lines")
    text, stats, _m, _p = H.run(whole, tmp_path, engine="device", device=hip_device, safe=True)
    assert text == H.EXPECTED["n3_forty_lines"]["expected"]["stdout"] and stats["host_lines"] == 0
    assert not (np.concatenate(stats["results"])["flags"] & nr.PASTE_UNSAFE).any()


def test_command_line_to_a_sorted_indexed_bgzf_file(tmp_path, hip_device):
    """N = 65: --engine device --bgzf --sort --tabix --deflate device, in a child process"""
    name = "n65_afreq_q_m"
    case = next(c for c in H.CASES if c["name"] == name)
    master, paths = P.write_case(case, str(tmp_path))
    listing = tmp_path / "list.txt"
    listing.write_text("".join(p + "\n" for p in paths))
    out = str(tmp_path / "cohort.vcf.gz")
    cmd = [sys.executable, "-m", "svtyper_amd.paste", "-f", str(listing), "-m", master, "-q", "--afreq", "--engine", "device", "--device",
           str(hip_device), "--bgzf", "--sort", "--tabix", "--deflate", "device", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    members = X.Members(raw)
    lines = members.text().split(b"\n")
    date = ("##fileDate=" + H.GOLDEN["file_date"]).encode()      # (the command line has no file_date: the line is the clock's)
    text = b"\n".join(date if l.startswith(b"##fileDate=") else l for l in lines)
    assert text == X.sorted_text(H.EXPECTED[name]["expected"]["stdout"].encode())
    tbi = X.read_tbi(open(out + ".tbi", "rb").read())
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(members.text(), n_random=50), members)

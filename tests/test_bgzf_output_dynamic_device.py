"""GPU: BGZF output in dynamic-Huffman blocks from the device -- the VCF of sso_genotype through
bgzf_out.open_text(deflate="device", huffman="dynamic"), and the `-w` BAM of the command line, `svtyper -w --reader device
--deflate device --huffman dynamic`, in child processes of their own: the inflated text and the inflated BAM stream are what
huffman="fixed" writes, byte for byte, and both files are smaller."""
import gzip
import os
import subprocess
import sys

import pytest

import test_host_pipeline as T
from svtyper_amd import bam, bgzf_out, singlesample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sso_vcf_in_dynamic_blocks(tmp_path, hip_device):
    raw = {}
    for huffman in ("fixed", "dynamic"):
        path = str(tmp_path / (huffman + ".vcf.gz"))
        out = bgzf_out.open_text(path, deflate="device", device=hip_device, huffman=huffman)
        with open(T.IN_VCF) as inf:
            singlesample.sso_genotype(T.IN_BAM, inf, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000)
        out.close()
        raw[huffman] = open(path, "rb").read()
    strip = lambda data: [l for l in data.split(b"\n") if not l.startswith(b"##fileDate")]
    assert strip(gzip.decompress(raw["dynamic"])) == strip(gzip.decompress(raw["fixed"]))
    assert raw["dynamic"].endswith(bam.BGZF_EOF) and raw["dynamic"][18] >> 1 & 3 == 2
    print("VCF: fixed %d bytes, dynamic %d bytes" % (len(raw["fixed"]), len(raw["dynamic"])))
    assert len(raw["dynamic"]) < len(raw["fixed"])


def test_command_line_write_alignment_in_dynamic_blocks(tmp_path, hip_device):
    env = dict(os.environ, PYTHONPATH=ROOT)
    raw = {}
    for huffman in ("fixed", "dynamic"):
        path = str(tmp_path / (huffman + ".bam"))
        r = subprocess.run([sys.executable, "-m", "svtyper_amd.classic", "-i", T.IN_VCF, "-B", T.IN_BAM, "-l", T.LIB_JSON, "-o", os.devnull, "-w", path,
                            "--reader", "device", "--deflate", "device", "--huffman", huffman], env=env, cwd=ROOT, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        raw[huffman] = open(path, "rb").read()
    assert gzip.decompress(raw["dynamic"]) == gzip.decompress(raw["fixed"]) and len(gzip.decompress(raw["fixed"])) > 100000
    assert raw["dynamic"].endswith(bam.BGZF_EOF)
    print("-w BAM: fixed %d bytes, dynamic %d bytes" % (len(raw["fixed"]), len(raw["dynamic"])))
    assert len(raw["dynamic"]) < len(raw["fixed"])

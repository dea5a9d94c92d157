"""GPU: BGZF output compressed on the device -- the VCF of sso_genotype through bgzf_out.open_text(deflate="device"), the `-w` BAM
of sv_genotype(reader="device", deflate="device"), both against the files deflate="host" writes, byte for byte; and the command
line, `--bgzf --deflate device`, in a child process of its own."""
import gzip
import os
import subprocess
import sys

import pytest

import test_host_pipeline as T
import test_write_alignment_device_reader as R
from svtyper_amd import bam, bgzf_out, singlesample

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sso_vcf_device_file_is_the_host_file(tmp_path, hip_device):
    raw = {}
    for deflate in ("host", "device"):
        path = str(tmp_path / (deflate + ".vcf.gz"))
        out = bgzf_out.open_text(path, deflate=deflate, device=hip_device)
        with open(T.IN_VCF) as inf:
            singlesample.sso_genotype(T.IN_BAM, inf, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000)
        out.close()
        raw[deflate] = open(path, "rb").read()
    assert raw["device"] == raw["host"] and raw["device"].endswith(bam.BGZF_EOF)
    strip = lambda text: [l for l in text.split("\n") if not l.startswith("##fileDate")]
    assert strip(gzip.decompress(raw["device"]).decode()) == strip(open(T.EXPECTED).read())


def test_write_alignment_device_file_is_the_host_file(tmp_path, hip_device):
    raw = {}
    for deflate in ("host", "device"):
        path = str(tmp_path / (deflate + ".bam"))
        R.run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, path, deflate=deflate)
        raw[deflate] = open(path, "rb").read()
    assert raw["device"] == raw["host"] and len(raw["device"]) > 100000


def test_command_line_bgzf_on_the_device(hip_device):
    common = [sys.executable, "-m", "svtyper_amd.singlesample", "-i", T.IN_VCF, "-B", T.IN_BAM, "-l", T.LIB_JSON]
    env = dict(os.environ, PYTHONPATH=ROOT)
    plain = subprocess.run(common, env=env, cwd=ROOT, capture_output=True, timeout=600)
    assert plain.returncode == 0, plain.stderr[-2000:]
    packed = subprocess.run(common + ["--bgzf", "--deflate", "device"], env=env, cwd=ROOT, capture_output=True, timeout=600)
    assert packed.returncode == 0, packed.stderr[-2000:]
    strip = lambda data: [l for l in data.split(b"\n") if not l.startswith(b"##fileDate")]
    assert packed.stdout[:4] == b"\x1f\x8b\x08\x04" and packed.stdout.endswith(bam.BGZF_EOF)
    assert strip(gzip.decompress(packed.stdout)) == strip(plain.stdout)


def test_command_line_bgzf_under_torch_distributed_run(tmp_path, hip_device):
    """two ranks: rank 0 alone wraps its output, and the file is one BGZF stream of the single-process text"""
    from test_sharded_drivers import _free_port
    single, multi = str(tmp_path / "single.vcf"), str(tmp_path / "multi.vcf.gz")
    common = ["-i", T.IN_VCF, "-B", T.IN_BAM, "-l", T.LIB_JSON]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    subprocess.run([sys.executable, "-m", "svtyper_amd.singlesample"] + common + ["-o", single], check=True, env=env, cwd=ROOT, timeout=600)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                    "--master-port", str(_free_port()), "-m", "svtyper_amd.singlesample"] + common + ["-o", multi, "--bgzf", "--deflate", "device"],
                   check=True, env=env, cwd=ROOT, timeout=900)
    raw = open(multi, "rb").read()
    strip = lambda data: [l for l in data.split(b"\n") if not l.startswith(b"##fileDate")]
    assert raw.endswith(bam.BGZF_EOF) and strip(gzip.decompress(raw)) == strip(open(single, "rb").read())

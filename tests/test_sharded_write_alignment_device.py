"""GPU: `svtyper -w FILE --gather-alignment` through the CLI under torch.distributed.run with two ranks (on a one-GPU box they
share the device and gather over gloo), against the same command in one process: the evidence BAM, its index and the VCF byte
for byte.  The records come from the device reader's dump and from the Python reader; rank 0 marks the first occurrences on the
GPU (svt_bam_first_device, since --deflate device) and the sorted writer makes the members and the CSI fold there.
(tests/test_sharded_write_alignment.py is the CPU side: gloo, the oracle engine.)"""
import os
import subprocess
import sys

import pytest

import test_host_pipeline as T
import test_sharded_drivers as S
import test_sharded_write_alignment as G
import verdictcases as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, in_path, name, flags, ranks):
    out_vcf, out_bam = str(tmp_path / (name + ".vcf")), str(tmp_path / (name + ".bam"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    launch = [sys.executable, "-m", "svtyper_amd.classic"]
    if ranks > 1:
        launch = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                  "--master-port", str(S._free_port()), "-m", "svtyper_amd.classic"]
        flags = flags + ["--gather-alignment"]
    subprocess.run(launch + ["-i", in_path, "-B", T.IN_BAM, "-l", T.LIB_JSON, "-o", out_vcf, "-w", out_bam] + flags, check=True, env=env,
                   cwd=ROOT, timeout=300 if ranks > 1 else 200)
    return out_vcf, out_bam


def _same(single, multi, index):
    for a, b in zip(single, multi):
        assert open(a, "rb").read() == open(b, "rb").read(), (a, b)
    assert open(single[1] + index, "rb").read() == open(multi[1] + index, "rb").read()
    other = ".bai" if index == ".csi" else ".csi"
    assert not os.path.exists(multi[1] + other) and not os.path.exists(single[1] + other)
    assert len(V.written_records(multi[1])[0]) >= 1000


def test_cli_two_ranks_write_the_one_process_files(tmp_path, hip_device):
    in_path, _n = G.make_input(tmp_path)
    # the device reader's dump, members and CSI fold on the GPU (a failing command raises: the second pair is then not started)
    flags = ["--reader", "device", "--deflate", "device", "--sort-alignment", "--alignment-csi"]
    _same(_run(tmp_path, in_path, "single_device", flags, 1), _run(tmp_path, in_path, "multi_device", flags, 2), ".csi")
    # the Python reader's reads through RecordSink.write
    flags = ["--reader", "python", "--deflate", "device", "--sort-alignment", "--bai"]
    _same(_run(tmp_path, in_path, "single_python", flags, 1), _run(tmp_path, in_path, "multi_python", flags, 2), ".bai")

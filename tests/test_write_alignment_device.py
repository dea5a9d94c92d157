"""GPU: `svtyper -w` through the HIP engine -- classic.sv_genotype(..., alignment_outpath=...) with the default engine, the XV
tags that depend on p_concordant and the small-deletion gate from svt_verdict_kernel -- gives the VCF bytes of the existing
goldens and, record for record and tag for tag, the BAM of tests/golden/write_alignment.json.gz (what the reference's own -w
code wrote; tests/test_write_alignment_host.py runs the same cases with the oracle standing in for the device)."""
import gzip
import io
import os

import pytest

import test_host_pipeline as T
import verdictcases as V
from svtyper_amd import classic

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_w(bams, vcf_path, lib_json, out_bam, **kw):
    out = io.StringIO()
    out.close = lambda: None
    with open(vcf_path) as inf:
        classic.sv_genotype(bams, inf, out, 20, 1, 1, 1000000, lib_json, False, out_bam, None, False, None, 1e10, **kw)
    return [l for l in out.getvalue().split("\n") if not l.startswith("##fileDate=")]


def same_writes(path, case):
    writes, mapq = V.written_records(path)
    assert len(writes) == len(case["writes"])
    for i, (got, want) in enumerate(zip(writes, case["writes"])):
        assert got == want, "record %d" % i
    assert mapq == case["mapq"]


def test_fixture_case_a(tmp_path, hip_device):
    out_bam = str(tmp_path / "a.bam")
    vcf = run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam)             # engine=None: the HIP engine; reader=None: "python" under -w
    assert vcf == [l for l in open(T.EXPECTED).read().split("\n") if not l.startswith("##fileDate=")]
    same_writes(out_bam, V.golden_cases()["a"])


def test_three_samples_blank_in_the_middle(tmp_path, hip_device):
    from svtyper_amd.pipeline import HipEngine
    from test_multisample_qual import three_sample_case
    bams, vcf_path, lib_json = three_sample_case(str(tmp_path))
    out_bam = str(tmp_path / "three_w.bam")
    vcf = run_w(bams, vcf_path, lib_json, out_bam, engine=HipEngine(hip_device, verdicts=True))
    assert vcf == gzip.open(os.path.join(HERE, "golden", "three.gt.vcf.gz"), "rt").read().split("\n")
    same_writes(out_bam, V.golden_cases()["three"])

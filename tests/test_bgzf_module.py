"""svtyper_amd/bgzf.py without a GPU: the BGZF layer under bam.py and bgzf_out.py is one module, the names bam.py always had
are the same objects, the payload per member is one constant, neither importer needs the other; and the one held close of the
two writers that hold their output (bgzf.close_held), where it refuses an index."""
import gzip
import os
import subprocess
import sys

import pytest

import baicases as B
import tbxcases as X
import test_bam_sort_host as H
from svtyper_amd import bam, bgzf, bgzf_out
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bam_re_exports_the_same_objects():
    assert bam.BgzfWriter is bgzf.BgzfWriter and bam.BgzfReader is bgzf.BgzfReader and bam.BGZF_EOF is bgzf.BGZF_EOF
    assert bam.check_deflate is bgzf.check_deflate and bam.check_huffman is bgzf.check_huffman
    assert bgzf_out.BgzfWriter is bgzf.BgzfWriter


def test_one_payload_constant():
    assert bgzf.PAYLOAD == nr.DEFLATE_MAX_PAYLOAD == X.PAYLOAD
    assert not hasattr(bam, "_BGZF_PAYLOAD") and not hasattr(bgzf_out, "_PAYLOAD")


@pytest.mark.parametrize("module", ["svtyper_amd.bgzf_out", "svtyper_amd.bam"])
def test_each_importer_alone_in_a_fresh_interpreter(module):
    r = subprocess.run([sys.executable, "-c", "import %s" % module], env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def junk(index_path):
    with open(index_path, "wb") as stale:
        stale.write(b"junk: an index of an earlier file")


def vcf_refusal(tmp_path):
    text = X.ORDERS["contig_reappears"]
    path = str(tmp_path / "u.vcf.gz")
    junk(path + ".tbi")
    out = bgzf_out.open_text(path, deflate="host", index="tbi")
    out.write(text.decode())
    return out, path, path + ".tbi", bgzf_out.VcfOrderError, ("line", X.first_out_of_order(text)), lambda raw: gzip.decompress(raw) == text


def bam_refusal(tmp_path):
    name = next(n for n in H.REFUSALS if B.CASES[n].refuse[0] == "order")
    case = B.CASES[name]
    path = str(tmp_path / "ev.bam")
    junk(path + ".bai")
    out = bam.AlignmentFile(path, "wb", template=H.Template(case.header), deflate="host", index="bai")
    for raw in case.records:
        out.write_raw(raw)
    return out, path, path + ".bai", bam.BamOrderError, ("record", case.refuse[1]), \
        lambda raw: gzip.decompress(raw) == case.header + b"".join(case.records)


@pytest.mark.parametrize("refusal", [vcf_refusal, bam_refusal])
def test_held_close_that_refuses_the_index(tmp_path, refusal):
    """index= without sort= over content that is not in order: the writer's own error, the data file complete, the index of
    an earlier file gone, and close() again does nothing"""
    out, path, index_path, error, (attribute, number), inflates_to_the_input = refusal(tmp_path)
    assert out._held is not None and os.path.exists(index_path)
    with pytest.raises(error) as e:
        out.close()
    assert type(e.value) is error and getattr(e.value, attribute) == number
    raw = open(path, "rb").read()
    assert raw.endswith(bgzf.BGZF_EOF) and inflates_to_the_input(raw)
    assert not os.path.exists(index_path)
    out.close()
    assert open(path, "rb").read() == raw and not os.path.exists(index_path)

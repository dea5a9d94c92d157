"""The inflate kernel (svt_inflate_kernel.h, one wavefront per BGZF member) against the same source on the CPU
(svt_bgzf_inflate_host): bytes and statuses are equal on every clean member and on the whole corruption corpus of
tests/test_inflate_host.py (which passes on the CPU first)."""
import numpy as np
import pytest

import inflatecases as I
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu


def _parity(members):
    data, block_off, out_off = I.layout([m for _label, m in members])
    host_out, host_status = nr.bgzf_inflate(data, block_off, out_off)
    dev_out, dev_status = nr.bgzf_inflate(data, block_off, out_off, device=0)
    bad = np.flatnonzero(host_status != dev_status)
    assert bad.size == 0, "statuses differ: %s" % [(members[k][0], int(host_status[k]), int(dev_status[k])) for k in bad[:8]]
    for k, (label, _m) in enumerate(members):
        if host_status[k] == 0:
            lo, hi = int(out_off[k]), int(out_off[k + 1])
            assert dev_out[lo:hi].tobytes() == host_out[lo:hi].tobytes(), label + ": bytes differ"
    return host_status


def test_zlib_members_equal_the_host_decoder(hip_device):
    status = _parity([(label, m) for label, m, _raw in I.zlib_members()])
    assert not status.any()


def test_members_of_the_walk_inputs_equal_the_host_decoder(hip_device, tmp_path):
    status = _parity([(label, m) for label, m, _raw in I.bam_members(I.walkcase_bams(tmp_path))])
    assert not status.any() and len(status) > 100


def test_corruption_corpus_equals_the_host_decoder(hip_device):
    corpus = I.corruption_corpus(I.bam_members([I.W.FIXTURE_BAM]))
    status = _parity(corpus)
    assert int(np.count_nonzero(status)) >= 200 and int(np.count_nonzero(status == 0)) >= 20


def test_no_members(hip_device):
    out, status = nr.bgzf_inflate(b"", np.zeros(0, np.uint64), np.zeros(1, np.uint64), device=0)
    assert len(out) == 0 and len(status) == 0

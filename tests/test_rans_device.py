"""The device twin of the rANS 4x8 decoder (svt_rans_kernel.h through svt_rans_decode_device) against the host twin: the whole
corpus of tests/cramcases.py in ONE batch, the malformed blocks among the others, with guard bytes around every output; and a
batch of 64 order-1 blocks of 4 099 bytes, so that several workgroups of the order-1 kernel run."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramcases as cc  # noqa: E402
import cramwriter as cw  # noqa: E402
from svtyper_amd import cram  # noqa: E402
from test_rans_host import FILL, GUARD, check_batch  # noqa: E402

pytestmark = pytest.mark.gpu


def test_device_equals_host_over_the_corpus_in_one_batch():
    corpus = cc.rans_corpus()
    blocks, sizes = [c[1] for c in corpus], [c[2] for c in corpus]
    h_out, h_off, h_status = cram.rans_decode(blocks, sizes, "host", guard=GUARD, fill=FILL)
    d_out, d_off, d_status = cram.rans_decode(blocks, sizes, "device", guard=GUARD, fill=FILL)
    assert np.array_equal(d_status, h_status), [(c[0], int(a), int(b)) for c, a, b in zip(corpus, d_status, h_status) if a != b]
    assert np.array_equal(d_off, h_off) and np.array_equal(d_out, h_out)
    assert check_batch(corpus, d_out, d_off, d_status) >= 12
    t = cram.rans_last_times()
    assert t["order0_kernel_s"] > 0 and t["order1_kernel_s"] > 0 and t["total_s"] > 0


def test_sixty_four_order1_blocks():
    rng = random.Random(7)
    plain = [bytes(rng.choice(b"ACGTNacgt,;:0123") for _ in range(4099)) for _ in range(64)]
    blocks = [cw.rans_encode(p, 1) for p in plain]
    assert all(b[0] == 1 for b in blocks)
    out, off, status = cram.rans_decode(blocks, [4099] * 64, "device", guard=GUARD, fill=FILL)
    assert not status.any()
    for p, o in zip(plain, off.tolist()):
        assert out[o:o + 4099].tobytes() == p
    guards = np.ones(out.shape[0], bool)
    for o in off.tolist():
        guards[o:o + 4099] = False
    assert (out[guards] == FILL).all()
    # without gaps between the outputs: the route a CRAM's blocks take
    out2, off2, status2 = cram.rans_decode(blocks, [4099] * 64, "device")
    assert not status2.any() and out2.tobytes() == b"".join(plain)

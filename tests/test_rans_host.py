"""The host twin of the rANS 4x8 decoder (svt_rans.h through svt_rans_decode_host) over the corpus of tests/cramcases.py, whose
blocks were made by the writer's own encoder: every well-formed block decodes to the bytes it was made from, every malformed one
gets its status and zeros, and in one batch no block touches the guard bytes around its neighbours' outputs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramcases as cc  # noqa: E402
from svtyper_amd import cram  # noqa: E402

GUARD, FILL = 24, 0xA5


def check_batch(corpus, out, off, status):
    """what both twins owe the corpus; -> the malformed blocks seen"""
    refused = 0
    guards = np.ones(out.shape[0], bool)
    for (name, _block, n, want, want_status), o, st in zip(corpus, off.tolist(), status.tolist()):
        got = out[o:o + n].tobytes()
        guards[o:o + n] = False
        if want_status is not None:
            assert st == want_status, (name, st)
        if want is not None:
            assert st == 0 and got == want, name
        if st:
            assert got == bytes(n), name            # a refused block's output range is zeroed
            refused += 1
    assert (out[guards] == FILL).all(), "a guard byte was written"
    assert int(guards.sum()) == GUARD * (len(corpus) + 1)
    return refused


def test_corpus_decodes_on_the_host():
    corpus = cc.rans_corpus()
    out, off, status = cram.rans_decode([c[1] for c in corpus], [c[2] for c in corpus], "host", guard=GUARD, fill=FILL)
    assert check_batch(corpus, out, off, status) >= 12
    sizes = {c[2] for c in corpus if c[4] == 0}
    assert {0, 1, 3, 4, 5, 4099} <= sizes
    assert {c[1][0] for c in corpus if c[4] == 0} == {0, 1}      # both orders among the well-formed


def test_each_malformed_block_alone_and_between_neighbours():
    corpus = cc.rans_corpus()
    good = next(c for c in corpus if c[0] == "text_o1")
    for case in corpus:
        if case[4] == 0:
            continue
        trio = [good, case, good]
        out, off, status = cram.rans_decode([c[1] for c in trio], [c[2] for c in trio], "host", guard=GUARD, fill=FILL)
        check_batch(trio, out, off, status)


def test_arguments_that_are_refused():
    import pytest
    from svtyper_amd import hip
    with pytest.raises(ValueError):
        cram.rans_decode([b""], [1], "gpu")
    with pytest.raises(ValueError):
        cram.rans_decode([b"", b""], [1], "host")
    out, off, status = cram.rans_decode([], [], "host")
    assert out.shape[0] == 0 and status.shape[0] == 0
    assert hip.ABI_VERSION == hip.load().svt_version()

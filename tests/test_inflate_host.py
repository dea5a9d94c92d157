"""The one-source DEFLATE decoder (svtyper_amd/csrc/svt_inflate.h) on the CPU, through svt_bgzf_inflate_host, against zlib: clean
BGZF members of every kind byte for byte, and a corruption corpus on which its verdict is raw zlib's for every case."""
import numpy as np

import inflatecases as I
from svtyper_amd import native_reads as nr


def _inflate_all(members, device=None):
    data, block_off, out_off = I.layout([m for _label, m in members])
    out, status = nr.bgzf_inflate(data, block_off, out_off, device)
    return out, status, out_off


def _check_clean(members, device=None):
    out, status, out_off = _inflate_all([(label, m) for label, m, _raw in members], device)
    for k, (label, _m, raw) in enumerate(members):
        assert status[k] == 0, "%s: status %d" % (label, status[k])
        assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == raw, label + ": bytes differ"
    return len(members)


def test_members_written_by_zlib_inflate_byte_for_byte():
    members = I.zlib_members()
    assert _check_clean(members) >= 46
    kinds = {label.split("/")[1] for label, _m, _r in members if "/" in label}
    assert kinds == {"l0", "l1", "l6", "l9", "fixed"}


def test_every_member_of_the_walk_inputs_inflates_byte_for_byte(tmp_path):
    members = I.bam_members(I.walkcase_bams(tmp_path))
    n = _check_clean(members)
    print("members", n, "bytes", sum(len(r) for _l, _m, r in members))
    assert n > 100


def test_member_layout_matches_the_python_header_walk():
    data = open(I.W.FIXTURE_BAM, "rb").read()
    block_off, out_off = nr.bgzf_members(data)
    members = I.file_members(I.W.FIXTURE_BAM)
    assert len(block_off) == len(members) and int(out_off[-1]) == sum(I.split_member(m)[1] for m in members)
    out, status = nr.bgzf_inflate(data, block_off, out_off)
    assert not status.any()
    assert out.tobytes() == b"".join(raw for _l, _m, raw in I.bam_members([I.W.FIXTURE_BAM]))


def test_corpus_floors_hold_for_zlib_alone():
    corpus = I.corruption_corpus(I.bam_members([I.W.FIXTURE_BAM]))
    verdicts = [I.reference(*I.split_member(m))[0] for _label, m in corpus]
    assert verdicts.count(False) >= 200 and verdicts.count(True) >= 20


def test_corruption_corpus_verdicts_are_zlibs():
    corpus = I.corruption_corpus(I.bam_members([I.W.FIXTURE_BAM]))
    out, status, out_off = _inflate_all(corpus)
    accepted, rejected = I.check_against_reference(corpus, out, status, out_off)
    print("corpus", len(corpus), "accepted", accepted, "rejected", rejected, "reasons",
          {nr.INFLATE_REASONS[r]: int(c) for r, c in zip(*np.unique(status[status != 0], return_counts=True))})
    assert rejected >= 200 and accepted >= 20


def test_argument_errors():
    import pytest
    from svtyper_amd import hip
    with pytest.raises(ValueError):
        nr.bgzf_inflate(b"", np.zeros(2, np.uint64), np.zeros(2, np.uint64))
    with pytest.raises(hip.SvtyperHipError):
        nr.bgzf_inflate(b"x" * 40, np.zeros(1, np.uint64), np.array([5, 0], np.uint64))
    out, status = nr.bgzf_inflate(b"x" * 40, np.zeros(1, np.uint64), np.array([0, 5], np.uint64))      # no member there
    assert status.tolist() == [9]
    out, status = nr.bgzf_inflate(b"", np.zeros(0, np.uint64), np.zeros(1, np.uint64))
    assert len(out) == 0 and len(status) == 0

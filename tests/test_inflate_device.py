"""The inflate kernel (svt_inflate_kernel.h, one wavefront per BGZF member) against the same source on the CPU
(svt_bgzf_inflate_host): bytes and statuses are equal on every clean member and on the whole corruption corpus of
tests/test_inflate_host.py (which passes on the CPU first).  Behind them the token corpus (tests/deflatewriter.py: streams no
compressor writes): the kernel's bytes against the truth and its statuses against the host's, bad members between clean ones of
odd sizes, and one call of more than 20 000 members twice.  What only the device can get wrong -- a missing sync mark, the
64-lane copies, the lane-striped table fill -- shows here as wrong bytes if the race is lost; that the marks are sufficient
is shown on the CPU by tests/test_inflate_marks.py."""
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


# ---- streams no compressor writes (tests/deflatewriter.py): against the truth, not only against the host build --------------------
def _device_matches_truth(entries, device_run=None):
    """entries: [(label, member, inflated bytes or None for a bad stream)].  The device's statuses are the host decoder's, a bad
    stream has one, and every good member's bytes are `raw`; -> (device bytes, statuses)"""
    data, block_off, out_off = I.layout([m for _label, m, _raw in entries])
    host_out, host_status = nr.bgzf_inflate(data, block_off, out_off)
    dev_out, dev_status = device_run or nr.bgzf_inflate(data, block_off, out_off, device=0)
    bad = np.flatnonzero(host_status != dev_status)
    assert bad.size == 0, "statuses differ: %s" % [(entries[k][0], int(host_status[k]), int(dev_status[k])) for k in bad[:8]]
    wrong = []
    for k, (label, _m, raw) in enumerate(entries):
        assert (dev_status[k] == 0) == (raw is not None), "%s: status %d" % (label, dev_status[k])
        if raw is not None and dev_out[int(out_off[k]):int(out_off[k + 1])].tobytes() != raw:
            wrong.append((k, label))
    assert not wrong, "bytes differ from the truth: %d members, first %s" % (len(wrong), wrong[:8])
    return dev_out, dev_status


def test_token_corpus_equals_the_truth(hip_device):
    entries = I.token_members() + [(label, m, None) for label, m in I.token_bad_members() + I.handmade_bad_members()]
    _out, status = _device_matches_truth(entries)
    assert int(np.count_nonzero(status == 0)) >= 60 and int(np.count_nonzero(status)) >= 23


def test_bad_members_between_clean_ones_of_odd_sizes(hip_device):
    """one call, bad members alternating with clean ones of ISIZE 1, 63, 65 and 65 535: a member that fails writes nothing
    outside its own place"""
    rnd = I.random.Random(63)
    clean = []
    for n in (1, 63, 65, 65535):
        raw = bytes(rnd.choice(b"ACGTN\n\t0123456789") if k % 7 else rnd.getrandbits(8) for k in range(n))
        clean.append(("clean%d" % n, I.member(I.deflate(raw), n, I.zlib.crc32(raw)), raw))
    bad = [(label, m, None) for label, m in I.token_bad_members() + I.handmade_bad_members()]
    entries = []
    for k, b in enumerate(bad):
        entries += [b, clean[k % 4]]
    _out, status = _device_matches_truth(entries)
    assert status[1::2].tolist() == [0] * len(bad) and np.count_nonzero(status[0::2]) == len(bad)


def test_twenty_thousand_members_in_one_call_twice(hip_device):
    entries = I.repeated_corpus()
    total = sum(I.split_member(m)[1] for _l, m, _r in entries)
    assert len(entries) >= 20000 and total <= 200_000_000
    assert {"eof", "isize65536/huffman/fixed", "isize65536/stored65000/dynamic"} <= {label for label, _m, _r in entries}
    out, status = _device_matches_truth(entries)
    data, block_off, out_off = I.layout([m for _label, m, _raw in entries])
    out2, status2 = nr.bgzf_inflate(data, block_off, out_off, device=0)
    _device_matches_truth(entries, (out2, status2))
    assert np.array_equal(status, status2)
    for k, (_label, _m, raw) in enumerate(entries):            # (a bad member's bytes are undefined: the good ones are compared)
        if raw is not None:
            lo, hi = int(out_off[k]), int(out_off[k + 1])
            assert np.array_equal(out[lo:hi], out2[lo:hi])
    print("members", len(entries), "inflated bytes", total, "bad", int(np.count_nonzero(status)))

"""GPU: svt_bam_first_device (svtyper_amd/csrc/svt_bam_first_kernel.h: the hash kernel, the record sort's radix passes over
(hash, index), the mark kernel) against the `set` restatement of tests/bamfirstcases.py and the host entry -- over the whole
corpus, around the sort's tile and the wavefront, with hashes cut down to 32, 4 and 1 bits so that distinct keys share runs,
on a stream long enough for several workgroups per kernel, and on malformed records.  That nothing is read outside a record's
span is what tests/test_bam_first_native.py checks: every access of the kernels goes through the same rules header."""
import numpy as np
import pytest

import bamfirstcases as F
from svtyper_amd import hip, native_reads as nr

pytestmark = pytest.mark.gpu

BITS = [64, 32, 4, 1]


@pytest.fixture(scope="module")
def corpus():
    return F.reach()


@pytest.fixture(scope="module")
def sized():
    """streams of n records for n around the wavefront (64) and kSortTile (1024), cut from one random stream and restated once"""
    spans = F.random_stream(2051, 23)
    out = {}
    for n in (63, 64, 65, 1023, 1024, 1025, 2051):
        data, off = F.stream(spans[:n])
        out[n] = (data, off, F.restate(spans[:n])[0], {bits: F.radix_passes(spans[:n], bits) for bits in BITS})
    return out


@pytest.mark.parametrize("hash_bits", BITS)
def test_the_corpus(hip_device, corpus, hash_bits):
    for name, spans in sorted(corpus.items()):
        data, off = F.stream(spans)
        want, want_bad = F.restate(spans)
        keep, bad = nr.bam_first(data, off, device=hip_device, hash_bits=hash_bits)
        host_keep, host_bad = nr.bam_first(data, off)
        assert bad == want_bad == host_bad, name                    # a malformed record: the host's number
        if want_bad:
            assert keep is None and host_keep is None, name
        else:
            assert keep.tolist() == want == host_keep.tolist(), name


@pytest.mark.parametrize("hash_bits", BITS)
def test_around_the_tile_and_the_wavefront(hip_device, sized, hash_bits):
    for n, (data, off, want, passes) in sized.items():
        keep, bad = nr.bam_first(data, off, device=hip_device, hash_bits=hash_bits)
        assert bad == 0 and keep.tolist() == want, n
        t = nr.bam_first_last_times()
        # the sort takes the digits in which the hashes differ, and no others: one with 1 or 4 bits, all eight with 64
        assert t["passes"] == passes[hash_bits] and (hash_bits > 4 or passes[hash_bits] == 1) and (hash_bits < 64 or passes[64] == 8), (n, t)


def test_a_long_stream_of_short_records(hip_device):
    spans = F.random_stream(70_000, 31, short=True)
    data, off = F.stream(spans)
    want = F.restate(spans)[0]
    assert 0.25 < want.count(0) / len(want) < 0.35
    keep, bad = nr.bam_first(data, off, device=hip_device)
    assert bad == 0 and np.array_equal(keep, np.array(want, np.uint8))
    t = nr.bam_first_last_times()
    print(t)
    assert t["passes"] == 8 and t["total_s"] > 0
    assert all(t[k] > 0 for k in ("hash_kernel_s", "histogram_kernel_s", "scan_kernel_s", "scatter_kernel_s", "mark_kernel_s"))
    host, _ = nr.bam_first(data, off)
    assert np.array_equal(keep, host)
    # a malformed record far into the stream, and two of them: the first one's number
    broken = list(spans)
    broken[65_537] = broken[65_537][:30]
    broken[1_234] = b""
    data, off = F.stream(broken)
    assert nr.bam_first(data, off, device=hip_device) == (None, 1_235)
    broken[1_234] = spans[1_234]
    data, off = F.stream(broken)
    assert nr.bam_first(data, off, device=hip_device) == (None, 65_538) == nr.bam_first(data, off)


def test_long_collision_runs(hip_device):
    """4 096 records, 16 hash values: runs of about 256 records, every lane walks its run to the front"""
    spans = F.random_stream(4096, 37)
    data, off = F.stream(spans)
    keep, bad = nr.bam_first(data, off, device=hip_device, hash_bits=4)
    assert bad == 0 and keep.tolist() == F.restate(spans)[0]
    assert nr.bam_first_last_times()["passes"] == F.radix_passes(spans, 4) == 1


def test_what_the_device_entry_refuses(hip_device, corpus):
    data, off = F.stream(corpus["all_unique"])
    for hash_bits in (0, 65, 1 << 31):
        with pytest.raises(hip.SvtyperHipError, match="hash_bits"):
            nr.bam_first(data, off, device=hip_device, hash_bits=hash_bits)
    back = off.copy()
    back[5], back[6] = off[6], off[5]
    with pytest.raises(hip.SvtyperHipError, match="must not decrease"):
        nr.bam_first(data, back, device=hip_device)
    keep, bad = nr.bam_first(b"", np.zeros(1, np.uint64), device=hip_device)          # n = 0 is legal
    assert bad == 0 and keep.shape == (0,)
    assert nr.bam_first(b"", np.zeros(3, np.uint64), device=hip_device) == (None, 1)
    # behind a header, and a table that runs past the bytes
    keep, bad = nr.bam_first(b"0123456789" + data, off + np.uint64(10), device=hip_device)
    assert bad == 0 and keep.tolist() == F.restate(corpus["all_unique"])[0]
    assert nr.bam_first(data[:-1], off, device=hip_device) == (None, len(off) - 1)

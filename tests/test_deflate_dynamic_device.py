"""GPU: the dynamic-Huffman mode on the device -- svt_bgzf_deflate_device_mode(SVT_DEFLATE_DYNAMIC) (svt_deflate_kernel<kDynamic>:
the token histogram by LDS atomics, the code built on the wavefront) against the host's dynamic bytes, byte for byte, over the
corpus of tests/dynhuffcases.py and 128 members of VCF text in one call; twice; its output through the device's own verified
inflate; svt_huffman_lengths_device against the host over the histograms, those deeper than the limit included; and the
refusals.  (tests/test_deflate_dynamic_host.py proves the host's bytes against the restatement of the format.)"""
import os

import numpy as np
import pytest

import deflatecases as D
import dynhuffcases as H
from svtyper_amd import hip
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def payloads():
    with open(os.path.join(HERE, "data", "example.gt.vcf"), "rb") as f:
        text = f.read()
    sizes = [D.MAX_PAYLOAD if k % 4 == 0 else 1 + (k * 7919) % D.MAX_PAYLOAD for k in range(128)]
    text = text * (sum(sizes) // len(text) + 1)
    out, at = [p for _name, p in H.corpus()], 0
    for size in sizes:
        out.append(text[at:at + size])
        at += size
    return out


@pytest.fixture(scope="module")
def host(payloads):
    return nr.bgzf_deflate(payloads, huffman="dynamic")


def test_device_bytes_are_the_hosts_twice_and_inflate_verified(hip_device, payloads, host):
    members, out_off = nr.bgzf_deflate(payloads, device=hip_device, huffman="dynamic")
    print(nr.bgzf_deflate_last_times())
    assert np.array_equal(out_off, host[1])
    differ = [k for k in range(len(payloads)) if not np.array_equal(members[int(out_off[k]):int(out_off[k + 1])], host[0][int(out_off[k]):int(out_off[k + 1])])]
    assert not differ, (len(differ), differ[:8], [len(payloads[k]) for k in differ[:8]])
    kinds = {int(members[int(out_off[k]) + 18]) >> 1 & 3 for k in range(len(payloads))}
    assert kinds == {0, 1, 2}                   # stored, fixed and dynamic blocks are all among them
    again, again_off = nr.bgzf_deflate(payloads, device=hip_device, huffman="dynamic")
    assert np.array_equal(again, members) and np.array_equal(again_off, out_off)
    sizes = np.array([0] + [len(p) for p in payloads], np.uint64)
    out, status = nr.bgzf_inflate(members.tobytes(), out_off[:-1], np.cumsum(sizes).astype(np.uint64), device=hip_device, verified=True)
    assert not status.any(), [(k, int(s)) for k, s in enumerate(status) if s][:8]
    assert out.tobytes() == b"".join(payloads)


def test_device_code_lengths_are_the_hosts(hip_device):
    for limit in (7, 15):
        sets = [f for _name, f, lim in H.histograms() if lim == limit]
        for symbols in sorted({len(f) for f in sets}):
            group = [f for f in sets if len(f) == symbols]
            freq = np.array(group * (2200 // len(group) + 1), np.uint32)       # (more histograms than a launch has waves: a wave takes several)
            want = nr.huffman_lengths(freq, limit)
            got = nr.huffman_lengths(freq, limit, device=hip_device)
            assert np.array_equal(got, want), (limit, symbols, np.argwhere(got != want)[:4].tolist())
    with pytest.raises(hip.SvtyperHipError):
        nr.huffman_lengths([1, 2, 3], 9, device=hip_device)


def test_refusals_on_the_device_route(hip_device):
    with pytest.raises(hip.SvtyperHipError, match="65280"):
        nr.bgzf_deflate([bytes(D.MAX_PAYLOAD + 1)], device=hip_device, huffman="dynamic")
    need = int(nr.bgzf_deflate([b"abc" * 100, b""], huffman="dynamic")[1][-1])
    assert need < int(nr.bgzf_deflate([b"abc" * 100, b""])[1][-1])
    with pytest.raises(hip.SvtyperHipError, match="capacity"):
        nr.bgzf_deflate([b"abc" * 100, b""], device=hip_device, capacity=need - 1, huffman="dynamic")
    members, out_off = nr.bgzf_deflate([b"abc" * 100, b""], device=hip_device, capacity=need, huffman="dynamic")
    assert members.size == need and list(nr.bgzf_deflate([], device=hip_device, huffman="dynamic")[1]) == [0]
    L = nr._lib()
    data, off = np.zeros(8, np.uint8), np.array([0, 8], np.uint64)
    out, out_off = np.full(64, 0xEE, np.uint8), np.zeros(2, np.uint64)
    rc = L.svt_bgzf_deflate_device_mode(data.ctypes.data, off.ctypes.data, 1, out.ctypes.data, out.size, out_off.ctypes.data, 2, int(hip_device))
    assert rc != 0 and (out == 0xEE).all()

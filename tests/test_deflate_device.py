"""GPU: svt_bgzf_deflate_device (svt_deflate_kernel.h: svtyper_amd/csrc/svt_deflate.h with one wavefront per member, the CRC-32
by svt_crc32_kernel, the members put side by side by svt_deflate_pack_kernel) against svt_bgzf_deflate_host, byte for byte, over
the whole corpus of tests/deflatecases.py and 512 members of VCF text in one call; twice; and its output through the device's
own verified inflate.  (tests/test_deflate_host.py proves the host's bytes against the restatement of the format.)"""
import os

import numpy as np
import pytest

import deflatecases as D
from svtyper_amd import hip
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def payloads():
    with open(os.path.join(HERE, "data", "example.gt.vcf"), "rb") as f:
        text = f.read()
    sizes = [D.MAX_PAYLOAD if k % 4 == 0 else 1 + (k * 7919) % D.MAX_PAYLOAD for k in range(512)]
    text = text * (sum(sizes) // len(text) + 1)
    out, at = [p for _name, p in D.corpus()], 0
    for size in sizes:
        out.append(text[at:at + size])
        at += size
    return out


@pytest.fixture(scope="module")
def host(payloads):
    return nr.bgzf_deflate(payloads)


def test_device_bytes_are_the_hosts_twice_and_inflate_verified(hip_device, payloads, host):
    members, out_off = nr.bgzf_deflate(payloads, device=hip_device)
    print(nr.bgzf_deflate_last_times())
    assert np.array_equal(out_off, host[1])
    differ = [k for k in range(len(payloads)) if not np.array_equal(members[int(out_off[k]):int(out_off[k + 1])], host[0][int(out_off[k]):int(out_off[k + 1])])]
    assert not differ, (len(differ), differ[:8], [len(payloads[k]) for k in differ[:8]])
    again, again_off = nr.bgzf_deflate(payloads, device=hip_device)
    assert np.array_equal(again, members) and np.array_equal(again_off, out_off)
    sizes = np.array([0] + [len(p) for p in payloads], np.uint64)
    out, status = nr.bgzf_inflate(members.tobytes(), out_off[:-1], np.cumsum(sizes).astype(np.uint64), device=hip_device, verified=True)
    assert not status.any(), [(k, int(s)) for k, s in enumerate(status) if s][:8]
    assert out.tobytes() == b"".join(payloads)


def test_refusals_on_the_device_route(hip_device):
    with pytest.raises(hip.SvtyperHipError, match="65280"):
        nr.bgzf_deflate([bytes(D.MAX_PAYLOAD + 1)], device=hip_device)
    need = int(nr.bgzf_deflate([b"abc" * 100, b""])[1][-1])
    with pytest.raises(hip.SvtyperHipError, match="capacity"):
        nr.bgzf_deflate([b"abc" * 100, b""], device=hip_device, capacity=need - 1)
    members, out_off = nr.bgzf_deflate([b"abc" * 100, b""], device=hip_device, capacity=need)
    assert members.size == need and list(nr.bgzf_deflate([], device=hip_device)[1]) == [0]

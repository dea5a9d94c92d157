"""svt_bgzf_deflate_host (svtyper_amd/csrc/svt_deflate.h on the CPU) against the Python restatement of the format
(tests/deflatecases.py), byte for byte over the whole corpus; its output inflated by zlib and by the project's own verified
inflate; the refusals of the C ABI; and a ratio guard, so that a build that stores everything cannot pass.  No GPU."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import deflatecases as D  # noqa: E402
from svtyper_amd import bam, hip  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402

DATA = os.path.join(HERE, "data")


@pytest.fixture(scope="module")
def cases():
    return D.corpus()


@pytest.fixture(scope="module")
def host(cases):
    """(members, out_off) of the corpus in one call"""
    return nr.bgzf_deflate([p for _name, p in cases])


def split(members, out_off):
    return [members[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(out_off) - 1)]


def chunks_of(data, size=D.MAX_PAYLOAD):
    return [data[i:i + size] for i in range(0, len(data), size)]


def test_the_corpus_reaches_what_the_format_names(cases):
    got = D.reach(cases)
    for key, want in D.REACH.items():
        assert not want - got[key], (key, sorted(want - got[key], key=str))


def test_host_bytes_are_the_restatements(cases, host):
    got = split(*host)
    assert len(got) == len(cases)
    for (name, p), member in zip(cases, got):
        assert member == D.member(p), name


def test_zlib_and_the_verified_inflate_return_the_payloads(cases, host):
    members, out_off = host
    for (name, p), member in zip(cases, split(members, out_off)):
        assert zlib.decompress(member[18:-8], -15) == p, name
        assert gzip.decompress(member) == p, name
    sizes = np.array([0] + [len(p) for _name, p in cases], np.uint64)
    out, status = nr.bgzf_inflate(members.tobytes(), out_off[:-1], np.cumsum(sizes).astype(np.uint64), verified=True)
    assert not status.any(), [(cases[k][0], int(s)) for k, s in enumerate(status) if s]
    assert out.tobytes() == b"".join(p for _name, p in cases)


def test_no_payload_is_the_eof_member():
    members, out_off = nr.bgzf_deflate([b""])
    assert members.tobytes() == bam.BGZF_EOF and list(out_off) == [0, 28]
    members, out_off = nr.bgzf_deflate([])
    assert members.size == 0 and list(out_off) == [0]


def test_payloads_inside_a_larger_buffer():
    data = bytes(range(256)) * 4
    off = np.array([100, 100, 400, 1024], np.uint64)
    members, out_off = nr.bgzf_deflate_at(data, off)
    assert split(members, out_off) == [D.member(b""), D.member(data[100:400]), D.member(data[400:1024])]


@pytest.mark.parametrize("what, text", [("long", "65280"), ("decreasing", "decrease"), ("capacity", "capacity")])
def test_refusals(what, text):
    if what == "long":
        call = lambda: nr.bgzf_deflate([bytes(D.MAX_PAYLOAD + 1)])
    elif what == "decreasing":
        call = lambda: nr.bgzf_deflate_at(bytes(100), np.array([0, 50, 40, 100], np.uint64), capacity=1000)
    else:
        need = int(nr.bgzf_deflate([b"abc" * 100, b""])[1][-1])
        call = lambda: nr.bgzf_deflate([b"abc" * 100, b""], capacity=need - 1)
        assert nr.bgzf_deflate([b"abc" * 100, b""], capacity=need)[0].size == need
    with pytest.raises(hip.SvtyperHipError, match=text):
        call()


def test_a_capacity_that_is_too_small_leaves_the_bytes_behind_it_alone():
    L = nr._lib()
    payload = np.frombuffer(b"abcd" * 300, np.uint8)
    off = np.array([0, 600, 1200], np.uint64)
    out = np.full(4096, 0xEE, np.uint8)
    out_off = np.zeros(3, np.uint64)
    need = int(nr.bgzf_deflate_at(payload.tobytes(), off)[1][-1])
    rc = L.svt_bgzf_deflate_host(payload.ctypes.data, off.ctypes.data, 2, out.ctypes.data, need - 1, out_off.ctypes.data)
    assert rc != 0 and (out[need - 1:] == 0xEE).all()


def ratio(payload):
    members, _off = nr.bgzf_deflate(chunks_of(payload))
    return members.size / len(payload)


def test_ratio_guard_on_vcf_text():
    with open(os.path.join(DATA, "example.gt.vcf"), "rb") as f:
        text = f.read()
    r = ratio(text)
    print("genotyped VCF text: %d bytes, members / payload = %.3f" % (len(text), r))
    assert r <= 0.55


def test_ratio_guard_on_the_fixture_bam_stream():
    with open(os.path.join(DATA, "NA12878.target_loci.sorted.bam"), "rb") as f:
        stream = gzip.decompress(f.read())
    r = ratio(stream)
    print("inflated BAM stream: %d bytes, members / payload = %.3f" % (len(stream), r))
    assert r <= 0.35

"""GPU: the BCF record kernels (svtyper_amd/csrc/svt_bcf_kernel.h) against the host twin, byte for byte -- records, offsets, spans,
refused line, kind and place -- at the smallest shapes where a lane-per-line kernel, its grid-stride loop and the member cut can
go wrong; svt_bcf_bgzf_device against the host route's stream and the host compressor's members; and the float envelope: no line
of the fixture's genotyped text or of the in-envelope corpus is handed to the host twin, every out-of-envelope token is, and the
result is the same."""
import os

import numpy as np
import pytest

import bcfcases as X
import bcfreader as R
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "data", "example.gt.vcf")
PAYLOAD = 65280


def same(host, dev):
    assert (dev["bad_line"], dev["bad_kind"], dev["bad_at"]) == (host["bad_line"], host["bad_kind"], host["bad_at"])
    for name in ("n_records", "header_len", "n_ref", "l_ref_max", "n_sample"):
        assert dev[name] == host[name], name
    if host["bad_line"]:
        assert "bytes" not in dev
        return
    assert dev["bytes"].tobytes() == host["bytes"].tobytes()
    assert dev["offsets"].tobytes() == host["offsets"].tobytes() and dev["spans"].tobytes() == host["spans"].tobytes()


def both(text, sort, device):
    data = text.encode()
    host, dev = nr.bcf_encode(data, sort=sort), nr.bcf_encode(data, sort=sort, device=device)
    same(host, dev)
    return host, dev


@pytest.mark.parametrize("n_lines", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_line_counts(hip_device, n_lines):
    host, dev = both(X.shaped_text(n_lines, 1), n_lines % 2 == 1, hip_device)
    assert host["n_records"] == n_lines and dev["host_lines"] == 0


@pytest.mark.parametrize("n_samples", [2, 63, 64, 65, 130])
def test_sample_counts(hip_device, n_samples):
    host, dev = both(X.shaped_text(5, n_samples), True, hip_device)
    assert host["n_sample"] == n_samples and dev["host_lines"] == 0
    _head, _d, records, _ = R.read_bcf(dev["bytes"].tobytes())
    assert len(records) == 5 and all(len(r["samples"]) == n_samples for r in records)


def test_corpus_and_envelope(hip_device):
    text = X.corpus_text()
    for sort in (False, True):
        _host, dev = both(text, sort, hip_device)
        assert dev["host_lines"] == sum(1 for _n, l in X.LINES if not X.line_in_envelope(l)) > 20
    _host, dev = both(X.corpus_text(envelope=True), False, hip_device)
    assert dev["host_lines"] == 0 and dev["n_records"] > 250
    # each out-of-envelope token on its own is handed over, and the result still matches
    outside = [(n, l) for n, l in X.LINES if not X.line_in_envelope(l)]
    for _name, line in outside[::3]:
        _host, dev = both(X.header() + X.LINES[1][1] + "\n" + line + "\n", False, hip_device)
        assert dev["host_lines"] == 1


def test_fixture_stays_on_the_device(hip_device):
    with open(FIXTURE) as f:
        text = f.read()
    _host, dev = both(text, True, hip_device)
    assert dev["host_lines"] == 0 and dev["n_records"] == 212
    times = nr.bcf_last_times()
    assert times["measure_kernel_s"] > 0 and times["write_kernel_s"] > 0 and times["total_s"] > 0


def test_refusals(hip_device):
    for _name, line, kind, _key in X.REFUSALS:
        for sort in (False, True):
            text = X.header() + X.LINES[1][1] + "\n" + X.LINES[2][1] + "\n" + line + "\n" + X.LINES[3][1] + "\n"
            host, _dev = both(text, sort, hip_device)
            assert host["bad_line"] == X.header().count("\n") + 3 and nr.BCF_KINDS[host["bad_kind"]] == kind
    # the lowest line number is the one reported, whichever lane finds its refusal first
    text = X.shaped_text(300, 1).split("\n")
    at = X.header().count("\n")
    for k in (290, 70, 200):
        text[at + k] = text[at + k].replace("SVTYPE=DEL", "NOPE=1")
    host, _dev = both("\n".join(text), False, hip_device)
    assert host["bad_line"] == at + 71


def boundary_text(exact):
    """a text whose third record ends exactly on the first member boundary (`exact`), or straddles it by one byte: the length of
    its EVENT string is found with the host twin (the descriptor of a long string takes a typed count of its own)"""
    lines = [l for _n, l in X.LINES if "\tGT" in l][:40]
    head = X.header() + lines[0] + "\n" + lines[1] + "\n"
    room = PAYLOAD - int(nr.bcf_encode(head.encode())["offsets"][-1])
    for n in range(room - 64, room):
        third = "chr2\t77\t.\tN\t<DEL>\t.\t.\tEVENT=%s\n" % ("e" * n)
        if int(nr.bcf_encode((head + third).encode())["offsets"][-1]) == PAYLOAD + (0 if exact else 1):
            return head + third + "".join(l + "\n" for l in lines[2:])
    raise AssertionError("no EVENT length puts the record's end on the boundary")


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
@pytest.mark.parametrize("exact", [True, False])
def test_members(hip_device, huffman, exact):
    text = boundary_text(exact)
    host = nr.bcf_encode(text.encode())
    ends = [int(o) for o in host["offsets"][1:]]
    assert (PAYLOAD in ends) == exact and (PAYLOAD + 1 in ends) != exact and ends[-1] > PAYLOAD
    dev = nr.bcf_bgzf_device(text.encode(), False, huffman, hip_device)
    stream = host["bytes"].tobytes()
    assert dev["spans"].tobytes() == host["spans"].tobytes() and dev["stream_len"] == len(stream)
    starts = [int(s) for s in dev["starts"]]
    assert starts == list(range(0, len(stream), PAYLOAD)) + [len(stream)]
    payloads = [stream[a:b] for a, b in zip(starts[:-1], starts[1:])]
    members, off = nr.bgzf_deflate(payloads, huffman=huffman)
    assert dev["bytes"].tobytes() == members.tobytes() and dev["offsets"].tobytes() == np.asarray(off, np.uint64).tobytes()
    assert R.stream_of(dev["bytes"].tobytes() + R.EOF) == stream


def test_sorted_members_and_long_lines(hip_device):
    """a joint-shaped text with lines far longer than a wavefront's 64 x 16 bytes, sorted, through the one call"""
    text = X.shaped_text(70, 130)
    lines = text.split("\n")
    at = X.header().count("\n")
    lines[at + 3] = lines[at + 3].replace("SVTYPE=DEL", "SVTYPE=DEL;EVENT=" + "long" * 2000)
    text = "\n".join(lines)
    host = nr.bcf_encode(text.encode(), sort=True)
    dev = nr.bcf_bgzf_device(text.encode(), True, "fixed", hip_device)
    assert dev["host_lines"] == 0 and R.stream_of(dev["bytes"].tobytes() + R.EOF) == host["bytes"].tobytes()
    assert dev["spans"].tobytes() == host["spans"].tobytes()

"""GPU: BCF records as VCF lines on the device (svtyper_amd/csrc/svt_bcf_text_kernel.h through svt_bcf_text_device: one wavefront per
record, lanes over samples) against the host twin, byte for byte: the text, the line offsets, the marks of the records the host
twin wrote (a float outside the device's envelope) and their count -- over the corpus of tests/bcfcases.py, its shaped texts
(sample counts around the wave's 64 lanes and its strides, record counts around a workgroup's four waves), the float edges, several
chunks, the hand-built IDX= file; the refusals the sanitised program (tests/test_bcf_text_native.py) has shown the shared rule to
refuse cleanly, with the same kind and record number; and svtyper_amd.update_info --engine device from a .bcf."""
import io

import numpy as np
import pytest

import bcfcases as X
import bcftextcases as C
import updateinfocases as K

from svtyper_amd import native_reads as nr
from svtyper_amd import update_info

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (5, 63), (5, 64), (5, 65), (3, 129), (2, 257), (3, 2), (4, 2), (5, 2))


def same(stream, device, block_bytes=None):
    """the device route's result is the host twin's under the device's float rule; -> it"""
    host = nr.bcf_text(stream, exact_floats=True, block_bytes=block_bytes)
    got = nr.bcf_text(stream, device=device, block_bytes=block_bytes)
    assert host["bad_record"] == 0 and got["bad_record"] == 0
    assert got["text"].tobytes() == host["text"].tobytes()
    assert np.array_equal(got["offsets"], host["offsets"]) and np.array_equal(got["marks"], host["marks"])
    for key in ("n_records", "header_len", "host_lines", "chunks", "n_sample", "text_len"):
        assert got[key] == host[key], key
    return got


def stream_of(text):
    return nr.bcf_encode(text.encode())["bytes"].tobytes()


def test_corpus(hip_device):
    got = same(stream_of(X.corpus_text()), hip_device)
    assert got["n_records"] == len(X.LINES) and 0 < got["host_lines"] < len(X.LINES) and got["chunks"] == 1
    times = nr.bcf_text_last_times()
    assert times["measure_kernel_s"] > 0 and times["write_kernel_s"] > 0 and times["total_s"] > 0


@pytest.mark.parametrize("n, s", SHAPES)
def test_shaped_texts(n, s, hip_device):
    assert same(stream_of(X.shaped_text(n, s)), hip_device)["n_records"] == n


def test_float_edges(hip_device):
    got = same(C.float_stream(C.edge_floats()), hip_device, block_bytes=16384)
    assert got["chunks"] > 1 and 200 < got["host_lines"] < got["n_records"] - 1000


def test_several_chunks(hip_device):
    stream = stream_of(X.corpus_text())
    assert same(stream, hip_device, block_bytes=4096)["chunks"] > 5
    wide = stream_of(X.shaped_text(5, 129))
    assert same(wide, hip_device, block_bytes=1)["chunks"] == 5


def test_idx_file(hip_device):
    stream, want = C.idx_stream()
    assert same(stream, hip_device)["text"].tobytes() == want.encode()


def test_refusals_are_the_host_twins(hip_device):
    for name, kind, bad in C.refusals():
        stream = C.refusal_stream(bad)
        host, got = nr.bcf_text(stream), nr.bcf_text(stream, device=hip_device)
        assert (got["bad_record"], got["bad_kind"]) == (host["bad_record"], host["bad_kind"]) == (2, got["bad_kind"]) and "text" not in got, name
        assert nr.BCF_TEXT_KINDS[got["bad_kind"]] == kind, name
    stream = stream_of(X.corpus_text())
    cut = nr.bcf_text(stream[:-5], device=hip_device, block_bytes=4096)
    assert cut["bad_record"] == len(X.LINES) and nr.BCF_TEXT_KINDS[cut["bad_kind"]] == "truncated"


def test_update_info_from_a_bcf_on_the_device(tmp_path, hip_device):
    from svtyper_amd import bcf_in, bcf_out
    case = K.bcf_case()
    path = str(tmp_path / "cohort.bcf")
    out = bcf_out.open_bcf(path)
    out.write(case["vcf"])
    out.close()
    stats = {}
    text = bcf_in.open_text(path, engine="device", device=hip_device, stats=stats).read()
    assert text == bcf_in.open_text(path).read() and stats["records"] == 5 and stats["times"]["write_kernel_s"] > 0
    want, got = io.StringIO(), io.StringIO()
    update_info.update_info(io.BytesIO(text), vcf_out=want, file_date="20240101", keep_contigs=True)
    update_info.update_info(path, vcf_out=got, engine="device", device=hip_device, file_date="20240101", keep_contigs=True)
    assert got.getvalue() == want.getvalue() and got.getvalue().count("\n") > 5

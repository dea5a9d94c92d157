"""First occurrences of a record stream on the host: svt_bam_first_host (svtyper_amd/csrc/svt_bam_first_rules.h) against the
`set` restatement of tests/bamfirstcases.py over the whole corpus, what the C entries refuse, bam.RecordSink against the file
writer byte for byte, and AlignmentFile.write_raw_many with a mask against a loop of write_raw.  No GPU here
(tests/test_bam_first_device.py is the device twin, tests/test_bam_first_native.py the sanitised program)."""
import ctypes as C
import os

import numpy as np
import pytest

import bamfirstcases as F
import test_host_pipeline as T
import test_write_alignment_walk_host as H
from svtyper_amd import bam, hip, native_reads as nr


@pytest.fixture(scope="module")
def corpus():
    return F.reach()


def test_the_host_entry_is_the_restatement(corpus):
    for name, spans in sorted(corpus.items()):
        data, off = F.stream(spans)
        want, want_bad = F.restate(spans)
        keep, bad = nr.bam_first(data, off)
        assert bad == want_bad, name
        assert (keep is None) if want_bad else (keep.dtype == np.uint8 and keep.tolist() == want), name


def test_the_records_may_lie_behind_a_header_and_apart(corpus):
    """rec_off[0] > 0 (what lies in front is nobody's record), and a last offset below the stream's length"""
    spans = corpus["random"]
    data, off = F.stream(spans)
    keep, bad = nr.bam_first(b"BAM\1header" + data + b"tail", off + np.uint64(10))
    assert bad == 0 and keep.tolist() == F.restate(spans)[0]
    # a table that runs past the bytes: the first record that does is no record
    keep, bad = nr.bam_first(data[:-1], off)
    assert keep is None and bad == len(spans)


def _raw_call(fn, data, off, n, keep, n_kept, bad, *more):
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    return fn(buf.ctypes.data, len(data), off.ctypes.data if off is not None else None, n, keep.ctypes.data if keep is not None else None,
              C.addressof(n_kept) if n_kept is not None else None, C.addressof(bad) if bad is not None else None, *more)


def test_what_the_c_entry_refuses(corpus):
    L = nr._need(*nr._FIRST)
    data, off = F.stream(corpus["all_unique"])
    n = len(off) - 1
    keep, n_kept, bad = np.zeros(n, np.uint8), C.c_uint64(7), C.c_uint64(7)
    assert _raw_call(L.svt_bam_first_host, data, off, n, keep, n_kept, bad) == 0 and (n_kept.value, bad.value) == (n, 0)
    assert _raw_call(L.svt_bam_first_host, data, off, 0, None, n_kept, bad) == 0 and (n_kept.value, bad.value) == (0, 0)     # n = 0 is legal
    invalid = hip.SVT_ERR_INVALID if hasattr(hip, "SVT_ERR_INVALID") else None
    back = off.copy()
    back[5], back[6] = off[6], off[5]
    for rc in (_raw_call(L.svt_bam_first_host, data, None, n, keep, n_kept, bad),
               _raw_call(L.svt_bam_first_host, data, off, n, None, n_kept, bad),
               _raw_call(L.svt_bam_first_host, data, off, n, keep, None, bad),
               _raw_call(L.svt_bam_first_host, data, off, n, keep, n_kept, None),
               _raw_call(L.svt_bam_first_host, data, back, n, keep, n_kept, bad),             # rec_off decreases
               _raw_call(L.svt_bam_first_host, data, off[:1], 1 << 32, keep, n_kept, bad)):   # refused before the table is read
        assert rc != 0 and (invalid is None or rc == invalid)
    with pytest.raises(hip.SvtyperHipError, match="must not decrease"):
        nr.bam_first(data, back)
    with pytest.raises(ValueError):
        nr.bam_first(data, np.zeros(0, np.uint64))


def test_abi_number_and_symbols():
    """added without a new ABI number: the three symbols are there to be probed for"""
    L = hip.load()
    assert L.svt_version() == hip.ABI_VERSION == 19
    assert all(hasattr(L, s) for s in ("svt_bam_first_host", "svt_bam_first_device", "svt_bam_first_last_times"))


# ------------------------------------------------------------------------------------------ RecordSink, write_raw_many
@pytest.fixture(scope="module")
def reads():
    """reads of the fixture BAM, some tagged the way `svtyper -w` tags them"""
    src = bam.AlignmentFile(T.IN_BAM, "rb")
    src._bgzf.seek(src._first_record)
    out = [src._next_record() for _ in range(3000)]
    for i, r in enumerate(out):
        if i % 3:
            r.set_tag("XV", "RA"[i % 2])
        r.query_sequence = None
    return src, out


def test_record_sink_holds_what_the_file_writer_writes(tmp_path, reads):
    src, rs = reads
    path = str(tmp_path / "file.bam")
    out, sink = bam.AlignmentFile(path, "wb", template=src), bam.RecordSink()
    raws = []
    for i, r in enumerate(rs):
        if i % 4 == 0:                                      # a finished record, as the device reader's dump hands them over
            raws.append(bam.record_of(r))
            out.write_raw(raws[-1])
            sink.write_raw(bytearray(raws[-1]))
        else:
            out.write(r)
            sink.write(r)
    out.close()
    sink.close()
    assert bytes(sink.data) == H.payload(path) and len(sink.offsets) == len(rs) + 1 and sink.offsets[-1] == len(sink.data)
    assert bytes(sink.data[sink.offsets[4]:sink.offsets[5]]) == raws[1]
    with pytest.raises(ValueError, match="one whole record"):
        bam.RecordSink().write_raw(raws[0][:-1])
    with pytest.raises(IOError):
        sink.write(rs[0])


@pytest.mark.parametrize("order", [{}, {"sort": True}, {"sort": True, "index": "bai"}, {"sort": True, "index": "bai", "csi": True},
                                   {"index": "bai"}], ids=["plain", "sorted", "sorted-bai", "sorted-csi", "bai"])
@pytest.mark.parametrize("deflate", ["host", "zlib"])
def test_write_raw_many_is_a_loop_of_write_raw(tmp_path, reads, order, deflate):
    src, rs = reads
    if order == {"index": "bai"}:
        rs = sorted(rs, key=lambda r: (r.reference_id, r.reference_start, r.is_reverse))    # (an index alone wants key order)
    sink = bam.RecordSink()
    for r in rs:
        sink.write(r)
    off = np.array(sink.offsets, np.uint64)
    rng = np.random.default_rng(3)
    masks = {"some": (rng.random(len(rs)) < 0.6).astype(np.uint8), "runs": np.repeat(rng.integers(0, 2, len(rs) // 50), 50).astype(np.uint8),
             "all": None, "none": np.zeros(len(rs), np.uint8)}
    for name, keep in masks.items():
        want, got = str(tmp_path / ("want_%s.bam" % name)), str(tmp_path / ("got_%s.bam" % name))
        a = bam.AlignmentFile(want, "wb", template=src, deflate=deflate, **order)
        for i in range(len(rs)):
            if keep is None or keep[i]:
                a.write_raw(sink.data[sink.offsets[i]:sink.offsets[i + 1]])
        a.close()
        b = bam.AlignmentFile(got, "wb", template=src, deflate=deflate, **order)
        b.write_raw_many(sink.data, off, keep)
        b.close()
        assert open(got, "rb").read() == open(want, "rb").read(), name
        for ext in (".bai", ".csi"):
            assert os.path.exists(got + ext) == os.path.exists(want + ext) == (order.get("index") is not None and (ext == ".csi") == bool(order.get("csi")))
            if os.path.exists(want + ext):
                assert open(got + ext, "rb").read() == open(want + ext, "rb").read(), name
    # two calls append; what write_raw refuses is refused for the whole call
    for kw in ({}, {"sort": True}):
        once, twice = str(tmp_path / "once.bam"), str(tmp_path / "twice.bam")
        a = bam.AlignmentFile(once, "wb", template=src, deflate=deflate, **kw)
        a.write_raw_many(sink.data, off)
        a.close()
        b = bam.AlignmentFile(twice, "wb", template=src, deflate=deflate, **kw)
        b.write_raw_many(sink.data, off[:1001])
        b.write_raw_many(sink.data, off[1000:])
        b.close()
        assert open(once, "rb").read() == open(twice, "rb").read()
        c = bam.AlignmentFile(str(tmp_path / "refused.bam"), "wb", template=src, deflate=deflate, **kw)
        with pytest.raises(ValueError):
            c.write_raw_many(sink.data, off[:4] + np.uint64(1))
        with pytest.raises(ValueError):
            c.write_raw_many(sink.data, off, np.ones(3, np.uint8))
        c.close()

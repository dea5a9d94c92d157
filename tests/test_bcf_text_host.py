"""BCF input on the host (svtyper_amd/csrc/svt_bcf_text.h through svt_bcf_text_host): the host twin of the record rule on the corpus
of tests/bcfcases.py and its shaped texts -- encoded by svt_bcf_encode_host, decoded, and held byte for byte to tests/bcftext.py over
the independent reader of tests/bcfreader.py; the exact float rule against snprintf and against Python's '%g' at its edges, with the
count of records the stated envelope leaves to the host; idempotence; chunks of one record; a hand-built file whose header carries
permuted and sparse IDX=; an empty body and a sites-only header; one test per refusal kind with its record number, a stream
truncated at every byte of its last record among them.  No GPU."""
import numpy as np
import pytest

import bcfcases as X
import bcfreader as R
import bcftext as T
import bcftextcases as C

from svtyper_amd import hip
from svtyper_amd import native_reads as nr

SHAPES = ((1, 1), (5, 63), (5, 64), (5, 65), (3, 129), (2, 257))


def stream_of(text):
    made = nr.bcf_encode(text.encode())
    assert made["bad_line"] == 0
    return made["bytes"].tobytes()


def decoded(stream, **kw):
    got = nr.bcf_text(stream, **kw)
    assert got["bad_record"] == 0, got
    return got


@pytest.fixture(scope="module")
def corpus():
    stream = stream_of(X.corpus_text())
    want, d, records = T.text(stream, R)
    return stream, want, d, records


def check_offsets(got, want):
    lines = want.splitlines(True)
    body = [l for l in lines if not l.startswith("#")]
    assert got["n_records"] == len(body) and got["header_len"] == len(want) - sum(map(len, body)) == got["offsets"][0]
    assert list(np.diff(got["offsets"].astype(np.int64))) == [len(l.encode()) for l in body] and got["offsets"][-1] == got["text_len"] == len(want.encode())


def test_corpus_is_the_yardsticks_text(corpus):
    stream, want, _d, records = corpus
    assert len(records) == len(X.LINES)
    got = decoded(stream)
    assert got["text"].tobytes() == want.encode()
    check_offsets(got, want)
    assert got["host_lines"] == 0 and not got["marks"].any() and got["chunks"] == 1 and got["n_sample"] == len(X.SAMPLES)


@pytest.mark.parametrize("n, s", SHAPES)
def test_shaped_texts(n, s):
    stream = stream_of(X.shaped_text(n, s))
    want = T.text(stream, R)[0]
    for kw in (dict(), dict(exact_floats=True), dict(block_bytes=1)):
        got = decoded(stream, **kw)
        assert got["text"].tobytes() == want.encode(), kw
        check_offsets(got, want)


def test_exact_floats_are_snprintfs_and_the_envelope_counts(corpus):
    """every float of the corpus prints the same by both rules; the records left to snprintf are those with a float outside
    0, -0, 1e-4 <= |x| < 1e6, by exact rational comparison"""
    stream, want, d, records = corpus
    plain, exact = decoded(stream), decoded(stream, exact_floats=True)
    assert exact["text"].tobytes() == plain["text"].tobytes() == want.encode()
    outside = [int(any(not T.in_envelope(b) for b in T.record_floats(rec, d))) for rec in records]
    assert 0 < sum(outside) < len(records)
    assert list(exact["marks"]) == outside and exact["host_lines"] == sum(outside)
    inside = sum(T.in_envelope(b) for rec in records for b in T.record_floats(rec, d))
    assert inside > 500                             # (what the comparison above is made on)


def test_exact_floats_at_the_edges_are_pythons():
    bits = C.edge_floats()
    want = C.FLOAT_HEADER + "".join("c\t%d\t.\tN\t.\t%s\t.\tV=%s\n" % (k + 1, T.float_text(b), T.float_text(b)) for k, b in enumerate(bits))
    plain, exact = decoded(C.float_stream(bits)), decoded(C.float_stream(bits), exact_floats=True)
    assert exact["text"].tobytes() == want.encode() and plain["text"].tobytes() == want.encode()
    assert list(exact["marks"]) == [int(not T.in_envelope(b)) for b in bits]
    assert 200 < exact["host_lines"] < len(bits) - 1000
    for value, text in ((0.0, "0"), (-0.0, "-0"), (999999.5, "1e+06"), (100000.5, "100000"), (100001.5, "100002"), (0.125, "0.125"), (285.53, "285.53")):
        k = bits.index(C.f32(value))
        assert T.float_text(bits[k]) == text and exact["marks"][k] == 0, value


def test_decode_encode_decode_is_the_same_text(corpus):
    stream, _want, _d, _records = corpus
    once = decoded(stream)["text"].tobytes()
    again = nr.bcf_encode(once)
    assert again["bad_line"] == 0
    assert decoded(again["bytes"].tobytes())["text"].tobytes() == once


def test_chunks_of_one_record(corpus):
    stream, want, _d, records = corpus
    got = decoded(stream, block_bytes=1)
    assert got["chunks"] == len(records) and got["text"].tobytes() == want.encode()
    some = decoded(stream, block_bytes=4096)
    assert 1 < some["chunks"] < len(records) and some["text"].tobytes() == want.encode()


def test_idx_permuted_and_sparse():
    stream, want = C.idx_stream()
    got = decoded(stream)
    assert got["text"].tobytes() == want.encode()
    head = want[:got["header_len"]]
    assert head == C.IDX_PRINTED and head.count("IDX=") == 1 and ",IDX=9 stays inside quotes" in head
    assert decoded(stream, exact_floats=True, block_bytes=1)["text"].tobytes() == want.encode()


def test_empty_body_and_sites_only_header():
    empty = stream_of(X.header())
    got = decoded(empty)
    assert got["n_records"] == 0 and got["chunks"] == 0 and got["text"].tobytes() == X.header().encode() and list(got["offsets"]) == [len(X.header())]
    sites = X.header(samples=()) + X.LINES[0][1] + "\n" + X.LINES[1][1] + "\n"
    stream = stream_of(sites)
    got = decoded(stream)
    assert got["n_sample"] == 0 and got["text"].tobytes() == T.text(stream, R)[0].encode()
    assert got["text"].tobytes().decode() == sites.replace("\t12.50\t", "\t12.5\t")     # (eight columns; QUAL printed by %g)


@pytest.mark.parametrize("name, kind, bad", C.refusals(), ids=[r[0] for r in C.refusals()])
def test_refusals(name, kind, bad):
    for kw in (dict(), dict(exact_floats=True, block_bytes=1)):
        got = nr.bcf_text(C.refusal_stream(bad), **kw)
        assert got["bad_record"] == 2 and nr.BCF_TEXT_KINDS[got["bad_kind"]] == kind and "text" not in got
    assert {r[1] for r in C.refusals()} == set(nr.BCF_TEXT_KINDS.values())


def test_the_lowest_refused_record_wins():
    refused = {r[0]: r[2] for r in C.refusals()}
    stream = C.stream(C.IDX_HEADER, [C.good_record(), refused["gt_as_characters"], refused["type_four"], C.good_record()])
    for block in (None, 1):
        got = nr.bcf_text(stream[:-3], block_bytes=block)
        assert got["bad_record"] == 2 and nr.BCF_TEXT_KINDS[got["bad_kind"]] == "gt"


def test_truncated_at_every_byte_of_the_last_record(corpus):
    stream, want, _d, records = corpus
    start = R.read_bcf(stream)[3][-1]
    for cut in range(start + 1, len(stream)):
        got = nr.bcf_text(stream[:cut])
        assert got["bad_record"] == len(records) and nr.BCF_TEXT_KINDS[got["bad_kind"]] == "truncated", cut
    assert decoded(stream[:start])["text"].tobytes() == "".join(want.splitlines(True)[:-1]).encode()


@pytest.mark.parametrize("stream, words", [(b"", "no BCF2.2 magic"), (b"BCF\2\1" + bytes(8), "no BCF2.2 magic"),
                                            (b"BCF\2\2\xff\0\0\0abc", "runs out of the stream"),
                                            (C.stream("##fileformat=VCFv4.2\n", []), "no #CHROM line"),
                                            (C.stream(C.IDX_HEADER.replace("IDX=4>", "IDX=3>"), []), "two IDs at one IDX")])
def test_a_stream_that_is_no_bcf_is_an_error(stream, words):
    with pytest.raises(hip.SvtyperHipError, match=words):
        nr.bcf_text(stream)

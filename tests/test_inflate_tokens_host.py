"""The one-source DEFLATE decoder (svtyper_amd/csrc/svt_inflate.h) on the CPU against streams no compressor writes: the token
corpus of tests/inflatecases.py, written by tests/deflatewriter.py.  Three things are checked: the writer and the plain reference
inflater against zlib (the authority), the decoder against the bytes zlib gives and against zlib's verdict on the bad streams, and
-- from the reference's profile alone, never from the decoder -- that the corpus reaches the edges it is named after."""
import numpy as np

import deflatewriter as D
import inflatecases as I
from svtyper_amd import native_reads as nr

_profiles = {}


def _profile(label, payload):
    if label not in _profiles:
        _profiles[label] = D.inflate(payload, I.MAX_ISIZE)
    return _profiles[label]


def _good_profiles():
    """[(label, bytes, Profile)] of the token members and of the payloads too large for a BGZF member"""
    out = []
    for label, m, _raw in I.token_members():
        ok, got, prof = _profile(label, I.split_member(m)[0])
        assert ok, label
        out.append((label, got, prof))
    for label, payload, _raw in I.oversize_payloads():
        ok, got, prof = _profile(label, payload)
        assert ok, label
        out.append((label, got, prof))
    return out


def test_reference_inflater_and_writer_agree_with_zlib():
    """bytes and verdict, on the token corpus (good, bad, oversize) and on what zlib's compressor writes"""
    n = 0
    for corpus, cached in ((I.token_members(), True), (I.zlib_members(), False)):
        for label, m, raw in corpus:
            payload, isize = I.split_member(m)
            ok, got, _prof = _profile(label, payload) if cached else D.inflate(payload, isize)
            assert I.reference(payload, isize) == (True, raw), label
            assert ok and got == raw and len(got) == isize, label
            n += 1
    for label, payload, raw in I.oversize_payloads():
        ok, got, _prof = _profile(label, payload)
        assert ok and got == raw == I.reference(payload, len(raw))[1], label
        n += 1
    for label, m in I.token_bad_members() + I.handmade_bad_members():
        payload, isize = I.split_member(m)
        ok, got, _prof = D.inflate(payload, isize)
        assert not I.reference(payload, isize)[0], label + ": zlib accepts"
        assert not (ok and len(got) == isize), label + ": the reference accepts"
        n += 1
    print("members", n)
    assert n >= 46 + 60 + 14 + 9


def test_decoder_inflates_the_token_corpus_byte_for_byte():
    members = I.token_members()
    data, block_off, out_off = I.layout([m for _label, m, _raw in members])
    out, status = nr.bgzf_inflate(data, block_off, out_off)
    for k, (label, _m, raw) in enumerate(members):
        assert status[k] == 0, "%s: status %d" % (label, status[k])
        assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == raw, label + ": bytes differ"
    assert len(members) >= 60


def test_decoder_verdicts_on_bad_token_streams_are_zlibs():
    bad = I.token_bad_members()
    # the same streams with nothing wrong next to them: a bad member's neighbours stay right
    mixed = [e for pair in zip(bad, [(label, m) for label, m, _raw in I.token_members()[:len(bad)]]) for e in pair]
    data, block_off, out_off = I.layout([m for _label, m in mixed])
    out, status = nr.bgzf_inflate(data, block_off, out_off)
    accepted, rejected = I.check_against_reference(mixed, out, status, out_off)
    reasons = {label: nr.INFLATE_REASONS[int(status[2 * k])] for k, (label, _m) in enumerate(bad)}
    print(reasons)
    assert rejected == len(bad) >= 14 and accepted == len(bad)
    # (the decoder's reason is the one the stream was built for)
    for label, reason in reasons.items():
        want = {"dist_beyond": "distance", "overrun_match": "output", "overrun_match_last": "output", "overrun_stored": "output",
                "incomplete15": "lengths", "single_dist_unused_code": "distance", "cut_in_distance_extra": "input"}[label.split("/")[1]]
        assert reason == want, (label, reason)


# ---- the corpus reaches what it names: conditions on the inputs, from the reference's profile -------------------------------------
def coverage():
    """the figures tests/inflatecases.py records in its docstring"""
    profiles = _good_profiles()
    matches = [m for _l, _b, p in profiles for m in p.matches]
    blocks = [b for _l, _b, p in profiles for b in p.blocks]
    huffman = [b for b in blocks if b["type"] != "stored"]
    lit_lens, dist_lens = {}, {}
    for b in huffman:
        for n, c in b["lit_code_lens"].items():
            lit_lens[n] = lit_lens.get(n, 0) + c
        for n, c in b["dist_code_lens"].items():
            dist_lens[n] = dist_lens.get(n, 0) + c
    full48 = 0
    for _l, _b, p in profiles:
        per_batch = {}
        for m in p.matches:
            if m.bits == 48:
                key = (m.block, m.index // I.BATCH)
                per_batch[key] = per_batch.get(key, 0) + 1
        full48 += sum(1 for c in per_batch.values() if c == I.BATCH)
    return {
        "members": len(profiles), "blocks": len(blocks), "matches": len(matches),
        "overlapping_matches": sum(1 for m in matches if m.dist < m.len),
        "overlap_distances": len({m.dist for m in matches if m.dist < m.len}),
        "cells": {(m.dist, m.len) for m in matches},
        "lit_code_lens": dict(sorted(lit_lens.items())), "dist_code_lens": dict(sorted(dist_lens.items())),
        "max_dist": max(m.dist for m in matches), "dist_32768": sum(1 for m in matches if m.dist == 32768),
        "isize_65536": sum(1 for _l, b, _p in profiles if len(b) == 65536),
        "eob_opens_a_batch": sum(1 for b in huffman if b["symbols"] > 0 and b["symbols"] % I.BATCH == 0),
        "empty_blocks": sum(1 for b in huffman if b["symbols"] == 0),
        "batches_of_128_48bit_symbols": full48,
        "stored_lens": sorted({b["stored_len"] for b in blocks if b["type"] == "stored"}),
        "lit_codes_over_fast_bits": sum(c for n, c in lit_lens.items() if n > 10),
        "dist_codes_over_fast_bits": sum(c for n, c in dist_lens.items() if n > 8),
    }


def test_the_corpus_reaches_what_it_names():
    c = coverage()
    print({k: v for k, v in c.items() if k != "cells"})
    missing = [cell for cell in I.overlap_cells() if cell not in c["cells"]]
    assert not missing, missing
    # every overlap distance 1..257 of the grid, not 1, 2, 3 and 8 alone
    assert c["overlap_distances"] >= len(I.OVERLAP_DISTS)
    for n in (9, 10, 11, 14, 15):
        assert c["lit_code_lens"].get(n, 0) > 0, "no literal/length code of %d bits" % n
    for n in (7, 8, 9, 14, 15):
        assert c["dist_code_lens"].get(n, 0) > 0, "no distance code of %d bits" % n
    assert c["max_dist"] == 32768 and c["dist_32768"] >= 10
    assert c["isize_65536"] >= 4
    # blocks of 128 and of 256 symbols under both codings, the 127-chain with its literal under both, the 48-bit batch
    assert c["eob_opens_a_batch"] >= 6
    assert c["empty_blocks"] >= 100
    assert c["batches_of_128_48bit_symbols"] >= 1
    assert 0 in c["stored_lens"] and 1 in c["stored_lens"] and 65535 in c["stored_lens"]
    assert I.MAX_PAYLOAD - 5 in c["stored_lens"]            # (the largest stored block a BGZF member holds)

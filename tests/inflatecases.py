"""Inputs shared by tests/test_inflate_host.py (CPU), tests/test_inflate_device.py (GPU) and the sanitizer run: clean BGZF
members, the corruption corpus made from them with a fixed seed, and the reference verdict (raw zlib inflate ends its stream
having produced exactly ISIZE bytes).

token_members() / token_bad_members() / oversize_payloads() are the streams no compressor writes, made from tokens by
tests/deflatewriter.py.  What the reference inflater's profile reports for them (tests/test_inflate_tokens_host.py, coverage();
64 members and the 2 payloads too large for a member; 14 bad streams besides): 638 blocks, 5 845 matches, 3 043 of them
overlapping at 257 different distances, all 295 (dist, len) cells of the overlap grid; literal/length codes decoded per length
1: 309, 2: 512, 3: 266, 4: 306, 5: 189, 6: 626, 7: 4 865, 8: 36 315, 9: 12 046, 10: 180, 11: 244, 14: 248, 15: 431 (923 beyond
the 10-bit table); distance codes 1: 557, 2: 563, 3: 94, 4: 1 590, 5: 2 603, 6: 10, 7: 52, 8: 45, 9: 50, 14: 52, 15: 229 (331
beyond the 8-bit table); distance 32 768 in 19 matches; 9 streams of ISIZE 65 536; 7 blocks whose end-of-block code opens a
batch; 203 blocks that are their end-of-block code alone; 1 batch of 128 symbols of 48 bits; stored blocks of LEN 0, 1, 21,
64, 32 768, 40 000, 65 000, 65 278, 65 505 (the largest a member holds) and 65 535 (oversize_payloads() only)."""
import functools
import random
import struct
import zlib

import numpy as np

import deflatewriter as D
import walkcases as W
from deflatewriter import BitWriter as _BitWriter

MAX_ISIZE = 65536


def member(payload, isize, crc=0):
    """a BGZF member around a raw-deflate payload"""
    bsize = len(payload) + 25
    assert bsize < 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize) + payload +
            struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(raw) + c.flush()
    return c.compress(raw[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[flush_at:]) + c.flush()


def split_member(m):
    """(payload, isize) of a member written by member() or found in a BAM"""
    xlen = m[10] | m[11] << 8
    return m[12 + xlen:len(m) - 8], struct.unpack("<I", m[-4:])[0]


def file_members(path):
    """the BGZF members of a file, as bytes each"""
    data = open(path, "rb").read()
    out, at = [], 0
    while at + 18 <= len(data):
        size = (data[at + 16] | data[at + 17] << 8) + 1
        out.append(data[at:at + size])
        at += size
    return out


def reference(payload, isize):
    """(ok, bytes): the verdict of raw zlib inflate"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, isize + 1)
    except zlib.error:
        return False, b""
    ok = d.eof and len(out) == isize
    return ok, out if ok else b""


def synthetic_inputs():
    rnd = random.Random(20261016)
    return {
        "random": bytes(rnd.getrandbits(8) for _ in range(30_000)),
        "all_equal": b"\x41" * 40_000,
        "period1": b"z" * 777,
        "period2": b"ab" * 9_000,
        "period3": b"xyz" * 7_001,
        "text": b"".join(b"read%05d\tchr%d\t%d\n" % (k, k % 23, rnd.randrange(10 ** 8)) for k in range(2_000)),
        "full_random": bytes(rnd.getrandbits(8) for _ in range(65_280)),
        "full_text": (b"ACGTTGCA" * 9000)[:65_280 - 300] + bytes(rnd.getrandbits(8) for _ in range(300)),
    }


LEVELS = (("l0", 0, zlib.Z_DEFAULT_STRATEGY), ("l1", 1, zlib.Z_DEFAULT_STRATEGY), ("l6", 6, zlib.Z_DEFAULT_STRATEGY),
          ("l9", 9, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED))


def zlib_members():
    """(label, member, inflated bytes): every synthetic input at levels 0 / 1 / 6 / 9 and with Z_FIXED, members of several
    deflate blocks, the EOF member"""
    out = []
    for name, raw in synthetic_inputs().items():
        for tag, level, strategy in LEVELS:
            out.append(("%s/%s" % (name, tag), member(deflate(raw, level, strategy), len(raw), zlib.crc32(raw)), raw))
    text = synthetic_inputs()["text"]
    for tag, level, strategy in LEVELS:
        out.append(("flush/%s" % tag, member(deflate(text, level, strategy, flush_at=len(text) // 3), len(text)), text))
    eof = member(b"\x03\x00", 0)
    assert len(eof) == 28
    out.append(("eof", eof, b""))
    return out


def bam_members(paths):
    out = []
    for path in paths:
        for k, m in enumerate(file_members(path)):
            payload, isize = split_member(m)
            out.append(("%s#%d" % (path.rsplit("/", 1)[-1], k), m, zlib.decompress(payload, -15)))
    return out


def walkcase_bams(tmp_path):
    """the BAMs tests/walkcases.py compares the readers on"""
    paths = [W.FIXTURE_BAM]
    for seed in W.SYNTHETIC_SEEDS[:3]:
        W.synthetic_input(tmp_path, seed)
        paths.append(str(tmp_path / ("syn%d.bam" % seed)))
    paths += [nbam.filename for _s, _sample, nbam in W.fake_inputs(tmp_path)]
    paths += [nbam.filename for _s, _sample, nbam in W.three_bam_inputs(tmp_path)]
    return paths


def handmade_bad_members():
    """streams no compressor writes: (label, member)"""
    btype3 = _BitWriter().bits(1, 1).bits(3, 2).done()
    # fixed block: length symbol 257 (7 bits 0000001), distance symbol 0 -- one byte back with nothing written yet
    before_start = _BitWriter().bits(1, 1).bits(1, 2).code(1, 7).code(0, 5).code(0, 7).done()
    # the same behind one literal 'a' (8 bits 0x30 + 0x61), distance symbol 1 = two bytes back
    before_start2 = _BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 0x61, 8).code(1, 7).code(1, 5).code(0, 7).done()
    # dynamic block whose code-length code has four codes of one bit
    over = _BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4)
    for _ in range(4):
        over.bits(1, 3)
    over = over.done() + b"\x00" * 8
    # ... and one with a single code-length code of two bits (incomplete)
    under = _BitWriter().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4).bits(2, 3).bits(0, 9).done() + b"\x00" * 8
    # fixed block using literal/length symbol 286 (8 bits 11000110) and distance symbol 30
    sym286 = _BitWriter().bits(1, 1).bits(1, 2).code(0xC6, 8).code(0, 7).done()
    dist30 = _BitWriter().bits(1, 1).bits(1, 2).code(0x30 + 0x61, 8).code(1, 7).code(30, 5).code(0, 7).done()
    stored_bad = _BitWriter().bits(1, 1).bits(0, 2).bits(0, 5).bits(3, 16).bits(0xFFFF, 16).done() + b"abc"
    return [("btype3", member(btype3, 0)), ("btype3/1", member(btype3, 1)), ("before_start", member(before_start, 3)),
            ("before_start2", member(before_start2, 4)), ("oversubscribed", member(over, 0)), ("incomplete", member(under, 0)),
            ("sym286", member(sym286, 0)), ("dist30", member(dist30, 4)), ("stored_nlen", member(stored_bad, 3))]


def corruption_corpus(fixture_members):
    """(label, member) made from 40 + clean members with a fixed seed: 8 single-bit flips, 2 truncated payloads and ISIZE one too
    large / one too small each, and the handmade streams"""
    rnd = random.Random(1016)
    clean = [(label, m) for label, m, _raw in zlib_members() if label.split("/")[0] in ("random", "all_equal", "period3", "text")]
    clean += [(label, m) for label, m, _raw in fixture_members[:20]]
    out = []
    for label, m in clean:
        payload, isize = split_member(m)
        for k in range(8):
            bit = rnd.randrange(len(payload) * 8)
            p = bytearray(payload)
            p[bit >> 3] ^= 1 << (bit & 7)
            out.append(("%s/flip%d" % (label, bit), member(bytes(p), isize)))
        for k in range(2):
            cut = rnd.randrange(1, len(payload))
            out.append(("%s/cut%d" % (label, cut), member(payload[:cut], isize)))
        out.append((label + "/isize+1", member(payload, isize + 1)))
        out.append((label + "/isize-1", member(payload, isize - 1)))
    return out + handmade_bad_members()


def layout(members):
    """(data, block_off, out_off) of members laid side by side; a member whose ISIZE no BGZF member can have gets no room"""
    data = b"".join(members)
    block_off = np.cumsum([0] + [len(m) for m in members[:-1]]).astype(np.uint64) if members else np.zeros(0, np.uint64)
    sizes = [split_member(m)[1] for m in members]
    out_off = np.cumsum([0] + [s if s <= MAX_ISIZE else 0 for s in sizes]).astype(np.uint64)
    return data, block_off, out_off


def check_against_reference(members, out, status, out_off):
    """every member: our verdict is the reference's, and where it is ok the bytes are equal; returns (accepted, rejected)"""
    accepted = rejected = 0
    for k, (label, m) in enumerate(members):
        payload, isize = split_member(m)
        ok, want = reference(payload, isize)
        assert (status[k] == 0) == ok, "%s: status %d, reference %s" % (label, status[k], "accepts" if ok else "rejects")
        if ok:
            assert out[int(out_off[k]):int(out_off[k + 1])].tobytes() == want, label + ": bytes differ"
            accepted += 1
        else:
            rejected += 1
    return accepted, rejected


# ---- the token corpus: streams no compressor writes (tests/deflatewriter.py) ------------------------------------------------------
MAX_PAYLOAD = 65510                            # BSIZE is 16 bits: a member is 65 536 bytes at most, 26 of them header and trailer
OVERLAP_DISTS = tuple(range(1, 10)) + (15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257)
CODINGS = ("fixed", "dynamic")
BATCH = 128                                    # svt::inf::kBatch


def overlap_cells():
    """the (dist, len) cells of the overlap grid"""
    return [(d, l) for d in OVERLAP_DISTS
            for l in sorted({min(258, max(3, x)) for x in (3, 4, d - 1, d, d + 1, 63, 64, 65, 127, 128, 129, 257, 258)})]


def _ladder(assign):
    """code lengths 1, 2, ..., 14, 15, 15 on the 16 symbols of `assign`"""
    assert sorted(assign.values()) == list(range(1, 16)) + [15]
    lengths = [0] * (max(assign) + 1)
    for s, l in assign.items():
        lengths[s] = l
    return lengths


_UNUSED_SHORT = {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 6, 6: 7, 7: 8, 8: 12, 9: 13}      # literals 0..9 are never written
# the symbols the tokens use sit on 9, 10, 11 (both sides of kFastBits = 10), 14 and 15
LIT_LADDER_A = _ladder({**_UNUSED_SHORT, **{97: 9, 98: 10, 99: 11, 100: 14, 256: 15, 257: 15}})
LIT_LADDER_B = _ladder({**_UNUSED_SHORT, **{97: 9, 98: 10, 258: 11, 285: 14, 256: 15, 99: 15}})
LIT_LADDER_C = _ladder({**_UNUSED_SHORT, **{259: 9, 256: 10, 97: 11, 98: 14, 99: 15, 260: 15}})
LIT_LADDER_MAX = _ladder({**_UNUSED_SHORT, **{97: 9, 98: 10, 99: 11, 100: 14, 256: 15, 284: 15}})
# distances: 7, 8, 9 (both sides of kDistFastBits = 8), 14 and 15; symbols 10..19 take the lengths nobody uses
DIST_LADDER = _ladder({10: 1, 11: 2, 12: 3, 13: 4, 14: 5, 15: 6, 0: 7, 1: 8, 2: 9, 16: 10, 17: 11, 18: 12, 19: 13, 3: 14, 4: 15, 29: 15})


def _huff(coding, tokens, **kw):
    return D.fixed(tokens) if coding == "fixed" else D.dynamic(tokens, **kw)


def _lits(rnd, n, lo=0, hi=256):
    return [rnd.randrange(lo, hi) for _ in range(n)]


def _mk(label, blocks):
    """(label, member, raw) of well-formed blocks; raw is zlib's output, and is what the tokens say"""
    payload = D.write(blocks)
    assert len(payload) <= MAX_PAYLOAD, (label, len(payload))
    raw = zlib.decompress(payload, -15)
    assert raw == D.expand(blocks) and len(raw) <= MAX_ISIZE, label
    return label, member(payload, len(raw), zlib.crc32(raw)), raw


def _random_tokens(rnd, n, pos):
    """n symbols, three literals to a match, behind `pos` bytes; -> (tokens, bytes they make)"""
    tokens, made = [], 0
    for _ in range(n):
        if pos + made >= 4 and rnd.random() < 0.25:
            t = (rnd.randrange(3, 24), rnd.randrange(1, min(pos + made, 300) + 1))
            made += t[0]
        else:
            t = rnd.randrange(256)
            made += 1
        tokens.append(t)
    return tokens, made


def _grid(rnd):
    out = []
    for coding in CODINGS:
        tokens, size, part = [], 0, 0
        for d, l in overlap_cells() + [(None, None)]:
            if d is None or size + d + l + 1 > 60000:
                out.append(_mk("grid/%s/%d" % (coding, part), [_huff(coding, tokens)]))
                tokens, size, part = [], 0, part + 1
            if d is not None:
                tokens += _lits(rnd, d) + [(l, d)] + _lits(rnd, 1)
                size += d + l + 1
    return out


def _chains(rnd):
    """dependence chains inside one batch; the batch starts with the block, so every pattern has a block of its own behind a
    block of literals to read from.  j: literals between the matches"""
    out = []
    for coding in CODINGS:
        for j in (0, 1, 2):
            tag = "%s/j%d" % (coding, j)
            # 127 matches in a row, each reading the last byte of the one before (dist >= j + 1, len >= dist); with j = 0 the
            # literal in front makes it one whole batch, and the end-of-block code the first symbol of the next
            tokens = _lits(rnd, 1)
            for k in range(127):
                dist = j + 2 + k % 4
                tokens += [(max(3, dist + k % 3), dist)] + _lits(rnd, j)
            out.append(_mk("chain/127/" + tag, [_huff(coding, _lits(rnd, 16)), _huff(coding, tokens)]))
            # M1; M2 reads M1 (even turns: marked) or older bytes (odd turns); M3 reads M1 alone, two matches back
            tokens = []
            for turn in range(30):
                m2 = (8, 4 + j) if turn % 2 == 0 else (8, 22 + j)
                tokens += [(8, 16)] + _lits(rnd, j) + [m2] + _lits(rnd, j) + [(8, 16 + 2 * j)] + _lits(rnd, j)
            out.append(_mk("chain/twoback/" + tag, [_huff(coding, _lits(rnd, 32)), _huff(coding, tokens)]))
            # M2's source: the last three bytes of M1 and the three literals between them
            tokens = []
            for turn in range(30):
                tokens += [(6, 10)] + _lits(rnd, 3) + [(8, 6)] + _lits(rnd, j)
            out.append(_mk("chain/straddle/" + tag, [_huff(coding, _lits(rnd, 16)), _huff(coding, tokens)]))
            # M1 is symbol 128 of its batch, M2 (reading M1) opens the next one behind j literals, M3 reads M2 inside that batch
            tokens = _lits(rnd, 127) + [(10, 50)] + _lits(rnd, j) + [(12, 5 + j)] + _lits(rnd, j) + [(5, 3 + j)] + _lits(rnd, 5)
            out.append(_mk("chain/split/" + tag, [_huff(coding, _lits(rnd, 16)), _huff(coding, tokens)]))
    return out


def _edges(rnd):
    out = []
    for coding in CODINGS:
        blocks, pos = [], 0
        for n in (127, 128, 129, 255, 256, 257):
            tokens, made = _random_tokens(rnd, n, pos)
            blocks.append(_huff(coding, tokens))
            pos += made
        out.append(_mk("edges/blocks/" + coding, blocks))
        empty = [_huff(coding, []) for _ in range(100)]
        out.append(_mk("edges/empty100/" + coding, [_huff(coding, _lits(rnd, 40))] + empty + [_huff(coding, _lits(rnd, 40) + [(30, 70)])]))
        out.append(_mk("edges/final_empty/" + coding, [_huff(coding, _lits(rnd, 200) + [(100, 150)]), _huff(coding, [])]))
    blocks, pos = [], 0
    for k in range(300):
        tokens, made = _random_tokens(rnd, 1 + k % 3, pos)
        blocks.append(D.stored(bytes(_lits(rnd, 1 + k % 3))) if k % 3 == 0 else _huff(CODINGS[k % 3 - 1], tokens))
        pos += 1 + k % 3 if k % 3 == 0 else made
    out.append(_mk("edges/tiny300", blocks))
    return out


def _from(rnd, n, choices, pos):
    """n tokens drawn from `choices` (a literal, or a length whose distance is drawn here)"""
    tokens = []
    for _ in range(n):
        c = rnd.choice(choices)
        if isinstance(c, tuple):
            c = (c[0], rnd.randrange(1, min(pos, 4000) + 1)) + c[1:]
            pos += c[0]
        else:
            pos += 1
        tokens.append(c)
    return tokens


def _code_lengths(rnd):
    out = []
    head = D.stored(bytes(_lits(rnd, 64)))
    out.append(_mk("codes/lit_ladder", [head,
                                        D.dynamic(_from(rnd, 400, [97, 98, 99, 100, (3,)], 64), lit_lengths=LIT_LADDER_A),
                                        D.dynamic(_from(rnd, 400, [97, 98, 99, (4,), (258, 285)], 64), lit_lengths=LIT_LADDER_B),
                                        D.dynamic(_from(rnd, 400, [97, 98, 99, (5,), (6,)], 64), lit_lengths=LIT_LADDER_C)]))
    # distance symbols 0, 1, 2, 3, 4 on 7, 8, 9, 14 and 15 bits (distances 1, 2, 3, 4 and 5..6)
    tokens = [(rnd.randrange(3, 40), rnd.choice((1, 2, 3, 4, 5, 6))) if k % 3 == 0 else rnd.randrange(256) for k in range(900)]
    out.append(_mk("codes/dist_ladder", [head, D.dynamic(tokens, dist_lengths=DIST_LADDER)]))
    for coding in CODINGS:
        tokens = _lits(rnd, 300)
        for k in range(40):
            tokens += [(257, 1 + k * 7, 284), (258, 300 - k, 285), (258, 2 + k, 284)] + _lits(rnd, 2)
        out.append(_mk("codes/len284_285/" + coding, [_huff(coding, tokens)]))
    # a batch of 128 symbols of 15 + 5 + 15 + 13 bits: length symbol 284 and distance symbol 29, both on 15-bit codes
    tokens = [(227 + k % 8, 32768 - k * 37 % 8000, 284) for k in range(BATCH)]
    out.append(_mk("codes/max48", [D.stored(bytes(_lits(rnd, 32768))), D.dynamic(tokens, lit_lengths=LIT_LADDER_MAX, dist_lengths=DIST_LADDER)]))
    tokens, _n = _random_tokens(rnd, 600, 0)
    out.append(_mk("codes/hlit286_hdist30_hclen19", [D.dynamic(tokens, header={"hlit": 286, "hdist": 30, "hclen": 19})]))
    out.append(_mk("codes/hclen19_no_repeats", [D.dynamic(tokens, header={"hclen": 19, "repeats": "none"})]))
    tokens = [(rnd.randrange(3, 259), 1) if k % 5 == 4 else rnd.randrange(256) for k in range(300)]
    out.append(_mk("codes/single_dist/sym0", [D.dynamic(tokens, dist_lengths=[1])]))
    tokens = _lits(rnd, 8) + [(rnd.randrange(3, 259), rnd.choice((7, 8))) if k % 5 == 4 else rnd.randrange(256) for k in range(300)]
    out.append(_mk("codes/single_dist/sym5", [D.dynamic(tokens, dist_lengths=[0, 0, 0, 0, 0, 1])]))
    out.append(_mk("codes/no_dist", [D.dynamic(_lits(rnd, 500), dist_lengths=[0])]))
    out.append(_mk("codes/eob_single_code", [D.dynamic(_lits(rnd, 10)), D.dynamic([], lit_lengths=[0] * 256 + [1], dist_lengths=[0])]))
    # a repeat of code lengths that runs from the literal/length lengths into the distance lengths: once a 16 (five sixes,
    # three of them literal/length symbols 283..285), once a run of zeros (18)
    lit = [0] * 286
    for s, l in {97: 1, 98: 2, 99: 3, 256: 4, 100: 6, 283: 6, 284: 6, 285: 6}.items():
        lit[s] = l
    dist = [6, 6, 5, 4, 3, 2, 1]
    tokens = _lits(rnd, 300, 97, 101)
    for k in range(60):
        tokens += [(rnd.choice((200, 240, 257, 258)), rnd.randrange(1, 13))] + _lits(rnd, 3, 97, 101)
    b16 = D.dynamic(tokens, lit_lengths=lit, dist_lengths=dist, header={"repeats": "greedy"})
    tokens = _lits(rnd, 100, 97, 105) + [(rnd.randrange(3, 11), rnd.randrange(50, 90)) for _ in range(50)]
    b18 = D.dynamic(tokens, header={"hlit": 286, "repeats": "greedy"})
    for b, sym in ((b16, 16), (b18, 18)):
        lit_l, _dist_l, ops, _cl, _hclen = D.dynamic_header(b)
        assert any(s == sym and lo < len(lit_l) < hi for (s, _e), (lo, hi) in zip(ops, D.op_spans(ops))), "no repeat across the boundary"
    out.append(_mk("codes/repeat_across_boundary", [b16, b18]))
    return out


def _stored(rnd):
    out = [_mk("stored/len0", [D.fixed(_lits(rnd, 20)), D.stored(b""), D.fixed(_lits(rnd, 20) + [(10, 30)])]),
           _mk("stored/len0_alone", [D.stored(b"")]),
           _mk("stored/len1", [D.stored(b"x"), D.fixed([(40, 1)]), D.stored(b"y")]),
           _mk("stored/largest_in_a_member", [D.stored(bytes(_lits(rnd, MAX_PAYLOAD - 5)))])]
    # a stored block behind a fixed block that ends at each of the eight bit positions: 3 + 8 a + 9 k + 7 bits
    blocks, seen = [], set()
    for k in range(8):
        first = D.fixed(_lits(rnd, 5, 0, 144) + _lits(rnd, k, 144, 256))
        seen.add(D.write_bits([first], final=False)[1] % 8)
        blocks += [first, D.stored(bytes(_lits(rnd, 21)))]
    assert seen == set(range(8))
    out.append(_mk("stored/behind_every_bit_alignment", blocks))
    for coding in CODINGS:
        tokens = [(258, 32768), (100, 40000 - 32768 + 258), (3, 1), (258, 32768), (17, 20000), (200, 32767), (90, 5000), (258, 2)]
        out.append(_mk("stored/reach/" + coding, [D.stored(bytes(_lits(rnd, 40000))), _huff(coding, tokens + _lits(rnd, 3) + [(258, 32768)])]))
    return out


def _sizes(rnd):
    out = []
    for coding in CODINGS:
        tokens = _lits(rnd, 300) + [(258, 1 + k * 113 % 300) for k in range(252)] + [(220, 7)]
        out.append(_mk("isize65536/huffman/" + coding, [_huff(coding, tokens)]))
        out.append(_mk("isize65536/stored65000/" + coding,
                       [D.stored(bytes(_lits(rnd, 65000))), _huff(coding, [(258, 32768), (258, 1000)] + _lits(rnd, 20))]))
        out.append(_mk("dist32768/at32768/stored/" + coding, [D.stored(bytes(_lits(rnd, 32768))), _huff(coding, [(258, 32768)] + _lits(rnd, 1))]))
        tokens = _lits(rnd, 256) + [(258, 1 + k * 61 % 256) for k in range(126)] + _lits(rnd, 4)
        out.append(_mk("dist32768/at32768/huffman/" + coding, [_huff(coding, tokens + [(258, 32768), (100, 32768)])]))
        tokens = _lits(rnd, 256) + [(258, 1 + k * 61 % 256) for k in range(252)] + _lits(rnd, 6)
        out.append(_mk("dist32768/at65278/huffman/" + coding, [_huff(coding, tokens + [(258, 32768)])]))
        out.append(_mk("dist32768/at65278/stored/" + coding, [D.stored(bytes(_lits(rnd, 65278))), _huff(coding, [(258, 32768)])]))
    for _label, _m, raw in out:
        assert len(raw) in (65536, 32768 + 259, 32768 + 358)
    return out


@functools.lru_cache(maxsize=None)
def _token_members():
    rnd = random.Random(20261017)
    return tuple(_grid(rnd) + _chains(rnd) + _edges(rnd) + _code_lengths(rnd) + _stored(rnd) + _sizes(rnd))


def token_members():
    """(label, member, inflated bytes): the overlap grid, dependence chains inside a batch, batch and block edges, code lengths
    up to 15 bits, stored blocks and the largest sizes, under fixed and under dynamic codes"""
    return list(_token_members())


@functools.lru_cache(maxsize=None)
def _oversize_payloads():
    rnd = random.Random(65535)
    big = bytes(_lits(rnd, 65535))
    out = []
    for label, blocks in (("stored/len65535", [D.stored(big)]), ("isize65536/stored65535+literal", [D.stored(big), D.fixed([big[7]])])):
        payload = D.write(blocks)
        raw = zlib.decompress(payload, -15)
        assert raw == D.expand(blocks)
        out.append((label, payload, raw))
    return tuple(out)


def oversize_payloads():
    """(label, payload, inflated bytes) of streams whose payload is larger than a BGZF member can hold (BSIZE is 16 bits: 65 510
    payload bytes): a stored block of LEN 65 535, and ISIZE 65 536 made from it and one literal.  svt_bgzf_inflate_host and
    _device take BGZF members, so these reach the decoder through tests/native/inflate_marks_main.cpp alone."""
    return list(_oversize_payloads())


@functools.lru_cache(maxsize=None)
def _token_bad_members():
    rnd = random.Random(7)
    out = []
    for coding in CODINGS:
        # a distance of out_pos + 1 as symbol k of a batch, behind matches of the same batch
        for k in (2, 64, 128):
            tokens, pos = [], 8
            for s in range(k - 1):
                tokens.append((3, 2) if s % 2 == 0 else rnd.randrange(256))
                pos += 3 if s % 2 == 0 else 1
            blocks = [_huff(coding, _lits(rnd, 8)), _huff(coding, tokens + [(3, pos + 1)] + _lits(rnd, 4))]
            out.append(("bad/dist_beyond/k%d/%s" % (k, coding), member(D.write(blocks), pos + 7)))
        # the output overrun by one byte by a match in the middle of a batch
        tokens, pos = [], 8
        for s in range(63):
            tokens.append((4, 3) if s % 3 == 0 else rnd.randrange(256))
            pos += 4 if s % 3 == 0 else 1
        blocks = [_huff(coding, _lits(rnd, 8)), _huff(coding, tokens + [(10, 5)] + _lits(rnd, 10))]
        out.append(("bad/overrun_match/" + coding, member(D.write(blocks), pos + 9)))
        out.append(("bad/overrun_match_last/" + coding, member(D.write([blocks[0], _huff(coding, tokens + [(10, 5)])]), pos + 9)))
    out.append(("bad/overrun_stored", member(D.write([D.fixed(_lits(rnd, 5)), D.stored(bytes(_lits(rnd, 100)))]), 104)))
    incomplete = list(LIT_LADDER_A)
    incomplete[257] = 0                        # 1, 2, ..., 14 and one code of 15 bits
    out.append(("bad/incomplete15", member(D.write([D.dynamic([97, 98, 99, 100], lit_lengths=incomplete)]), 4)))
    blocks = [D.dynamic([97, 98, ("litsym", 257), ("bits", 1, 1)] + _lits(rnd, 20), dist_lengths=[1])]       # (bits behind it: not the end of the input)
    out.append(("bad/single_dist_unused_code", member(D.write(blocks), 25)))
    # the payload ends inside the 13 extra bits of a distance: the match is the last symbol in front of a 15-bit end-of-block code
    blocks = [D.stored(bytes(_lits(rnd, 32768))), D.dynamic([97, (230, 32768 - 1234, 284)], lit_lengths=LIT_LADDER_MAX, dist_lengths=DIST_LADDER)]
    payload, nbits = D.write_bits(blocks)
    cut = (nbits - 15 - 1) // 8
    assert nbits - 15 - 13 < 8 * cut < nbits - 15
    out.append(("bad/cut_in_distance_extra", member(payload[:cut], 32768 + 231)))
    return tuple(out)


def token_bad_members():
    """(label, member): bad streams made from tokens; the verdict is raw zlib's"""
    return list(_token_bad_members())


def repeated_corpus(n_min=20000, max_bytes=200_000_000, seed=20261017):
    """[(label, member, inflated bytes or None)]: one call of at least n_min members and at most max_bytes inflated -- every
    token member, the bad ones, the EOF member and the 65 536-byte members among them, the small members repeated most,
    shuffled with a fixed seed"""
    good = token_members() + [e for e in zlib_members() if e[0] == "eof"]
    entries = [(label, m, raw) for label, m, raw in good] + [(label, m, None) for label, m in token_bad_members()]
    size = lambda e: split_member(e[1])[1]
    big = [e for e in entries if size(e) > 4096]
    small = [e for e in entries if size(e) <= 4096]
    budget = max_bytes * 3 // 4
    big_reps = max(1, min(40, budget // 2 // max(1, sum(size(e) for e in big))))
    small_reps = -(-(n_min - big_reps * len(big)) // len(small))
    out = big * big_reps + small * small_reps
    assert len(out) >= n_min and sum(size(e) for e in out) <= max_bytes
    random.Random(seed).shuffle(out)
    return out

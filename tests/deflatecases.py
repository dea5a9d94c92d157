"""The BGZF deflate format of DESIGN 3.4, restated in Python, and the corpus the deflate tests share: pure Python, test code only.

Restatement.  parse(p) is the cut into 64 chunks and the greedy parse of each over its own table (a dict under the hash: the
same entries a table of 2^T_BITS slots holds, since a slot is only ever found through its hash); cdata(p) writes the tokens
with deflatewriter.fixed, or deflatewriter.stored where the fixed block is no gain; member(p) puts the header bam.BgzfWriter
writes, the CRC-32 and ISIZE around it.  Nothing here looks at the code under test.

Corpus.  corpus() is [(name, payload)], built once; reach(corpus) is what the restatement's own tokens say the corpus reaches,
and REACH is what it has to reach (tests/test_deflate_host.py asserts it)."""
import functools
import random
import struct
import zlib

import deflatewriter as dw

LANES, MAX_PAYLOAD, T_BITS = 64, 65280, 8
HEADER = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


def _hash(p, i):
    return ((int.from_bytes(p[i:i + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - T_BITS)


def parse(p):
    """the tokens of the 64 chunks: [[literal | (length, distance, source, position)]]"""
    n = len(p)
    c = -(-n // LANES)
    chunks = []
    for lane in range(LANES):
        a, b = min(n, lane * c), min(n, (lane + 1) * c)
        table, tokens = {}, []
        for i in range(max(0, a - c), a):
            if i + 4 <= n:
                table[_hash(p, i)] = i
        i = a
        while i < b:
            m, j = 0, None
            if i + 4 <= n:
                j, lim = table.get(_hash(p, i)), min(258, b - i)
                if j is not None and lim >= 4 and p[j:j + 4] == p[i:i + 4]:
                    m = 4
                    while m < lim and p[j + m] == p[i + m]:
                        m += 1
            if m:
                tokens.append((m, i - j, j, i))
                for k in range(i, i + m):
                    if k + 4 <= n:
                        table[_hash(p, k)] = k
                i += m
            else:
                tokens.append(p[i])
                if i + 4 <= n:
                    table[_hash(p, i)] = i
                i += 1
        chunks.append(tokens)
    return chunks


def token_bits(t):
    if isinstance(t, int):
        return 8 if t < 144 else 9
    s, d = dw.length_symbol(t[0]), dw.distance_symbol(t[1])
    return (7 if s < 280 else 8) + dw.LENGTH_EXTRA[s - 257] + 5 + dw.DIST_EXTRA[d]


def fixed_bytes(chunks):
    """F: the bytes of the fixed block"""
    return (3 + sum(token_bits(t) for tokens in chunks for t in tokens) + 7 + 7) // 8


def cdata(p, chunks=None):
    chunks = parse(p) if chunks is None else chunks
    n = len(p)
    if n > 0 and fixed_bytes(chunks) >= 5 + n:
        return dw.write([dw.stored(p)])
    out = dw.write([dw.fixed([t if isinstance(t, int) else t[:2] for tokens in chunks for t in tokens])])
    assert len(out) == fixed_bytes(chunks)
    return out


def member(p, chunks=None):
    c = cdata(p, chunks)
    return HEADER + struct.pack("<H", len(c) + 25) + c + struct.pack("<II", zlib.crc32(p) & 0xFFFFFFFF, len(p))


# ---- the corpus ------------------------------------------------------------------------------------------------------------------
LENGTH_BASES = dw.LENGTH_BASE[1:]            # the first length of every symbol 258 .. 285 (4 .. 258)
N_DIST_SYMBOLS = 22                          # distances stay below 2 C <= 2040: symbols 0 .. 21


def _text(n, seed):
    """VCF-like lines: repeats at many distances, all bytes below 144"""
    r = random.Random(seed)
    out = bytearray()
    pos = 10000
    while len(out) < n:
        pos += r.randrange(1, 4000)
        gts = "\t".join("%s:%d:%d:%.2f" % (r.choice(("0/0", "0/1", "1/1", "./.")), r.randrange(40), r.randrange(200), r.random() * 90)
                        for _ in range(r.randrange(1, 5)))
        out += ("chr%d\t%d\t%d\tN\t<%s>\t%.2f\t.\tSVTYPE=%s;END=%d\tGT:GQ:DP:AB\t%s\n"
                % (r.randrange(1, 23), pos, r.randrange(9999), r.choice(("DEL", "DUP", "INV")), r.random() * 1000,
                   r.choice(("DEL", "DUP", "BND")), pos + r.randrange(50, 9000), gts)).encode()
    return bytes(out[:n])


def _mostly_low(n, high, seed):
    """n bytes below 144 but for `high` of them: literals of 8 and of 9 bits, so that the lanes' bits begin anywhere in a byte"""
    r = random.Random(seed)
    out = bytearray(r.randrange(144) for _ in range(n))
    for i in r.sample(range(n), min(high, n)):
        out[i] = r.randrange(144, 256)
    return bytes(out)


def _periodic(period, n, seed, low=0, high=256):
    r = random.Random(seed)
    unit = bytes(r.randrange(low, high) for _ in range(period))
    return (unit * (n // period + 1))[:n]


@functools.lru_cache(maxsize=None)
def corpus():
    r = random.Random(20240521)
    out = []
    for n in range(131):                     # every length 0 .. 130: C = 1 with empty lanes, C = 2, C = 3 -- literals only
        out.append(("low-%d" % n, _mostly_low(n, n % 20, n)))
        out.append(("random-%d" % n, bytes(r.randrange(256) for _ in range(n))))
    out.append(("edge-fixed", _mostly_low(64, 22, 1)))         # F = 4 + n: the last payload that stays a fixed block ...
    out.append(("edge-stored", _mostly_low(64, 23, 1)))        # ... and F = 5 + n: the first that is stored
    for n in (1019, 1020, 1021):
        out.append(("text-%d" % n, _text(n, n)))
    for n in (65279, 65280):
        out.append(("text-%d" % n, _text(n, n)))
    for n in (63, 300, 1021, 64 * 313, 65280):                 # distance 1; lengths clamped by 258 and by the chunk's end
        out.append(("zero-%d" % n, bytes(n)))
    out.append(("high-10", _mostly_low(10, 10, 2)))            # literals of 9 bits only, in a fixed block
    out.append(("high-1000", _periodic(7, 1000, 3, 144, 256)))
    for c in LENGTH_BASES:                                     # lanes 1 .. 63 hold one match of the chunk's length each
        out.append(("period-%d-length-%d" % (1 + c % 3, c), _periodic(1 + c % 3, 64 * c, c)))
    for s in range(N_DIST_SYMBOLS):                            # the first distance of every symbol, as a period of random bytes
        d = dw.DIST_BASE[s]
        out.append(("distance-%d" % d, _periodic(d, 64 * min(1020, max(4, d + 6)), 100 + s)))
    out.append(("random-1000", bytes(r.randrange(256) for _ in range(1000))))
    out.append(("random-65280", bytes(r.randrange(256) for _ in range(65280))))
    return tuple(out)


REACH = {
    "lengths": set(range(131)) | {1019, 1020, 1021, 65279, 65280},
    "length_symbols": set(range(258, 286)),
    "distance_symbols": set(range(N_DIST_SYMBOLS)),
    "flags": {"empty-lanes", "distance-1", "length-258", "length-to-chunk-end", "nine-bit-literals-only", "source-in-chunk-before", "stored",
              "fixed", "edge-fixed", "edge-stored", "shared-byte"},
}


def reach(cases):
    """what the restatement's tokens say `cases` reach, in the terms of REACH"""
    got = {"lengths": set(), "length_symbols": set(), "distance_symbols": set(), "flags": set()}
    for _name, p in cases:
        n = len(p)
        c = -(-n // LANES)
        chunks = parse(p)
        f = fixed_bytes(chunks)
        stored = n > 0 and f >= 5 + n
        got["lengths"].add(n)
        got["flags"].add("stored" if stored else "fixed")
        if n and f == 5 + n:
            got["flags"].add("edge-stored")
        if n and f == 4 + n:
            got["flags"].add("edge-fixed")
        if stored:
            continue
        if 0 < n < LANES:
            got["flags"].add("empty-lanes")
        literals = [t for tokens in chunks for t in tokens if isinstance(t, int)]
        if literals and all(t >= 144 for t in literals):
            got["flags"].add("nine-bit-literals-only")
        at = 3
        for lane, tokens in enumerate(chunks):
            bits = sum(token_bits(t) for t in tokens)
            if bits and at % 8:
                got["flags"].add("shared-byte")
            at += bits
            for t in tokens:
                if isinstance(t, int):
                    continue
                m, d, j, i = t
                got["length_symbols"].add(dw.length_symbol(m))
                got["distance_symbols"].add(dw.distance_symbol(d))
                if d == 1:
                    got["flags"].add("distance-1")
                if m == 258:
                    got["flags"].add("length-258")
                if m < 258 and i + m == min(n, (lane + 1) * c) and i + m < n and p[j + m] == p[i + m]:
                    got["flags"].add("length-to-chunk-end")
                if j + m <= lane * c:
                    got["flags"].add("source-in-chunk-before")
    return got

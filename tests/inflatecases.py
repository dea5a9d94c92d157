"""Inputs shared by tests/test_inflate_host.py (CPU), tests/test_inflate_device.py (GPU) and the sanitizer run: clean BGZF
members, the corruption corpus made from them with a fixed seed, and the reference verdict (raw zlib inflate ends its stream
having produced exactly ISIZE bytes)."""
import random
import struct
import zlib

import numpy as np

import walkcases as W

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


class _BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def bits(self, value, count):              # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += count
        return self

    def code(self, value, count):              # a Huffman code: first bit of the code first
        for k in range(count - 1, -1, -1):
            self.bits(value >> k & 1, 1)
        return self

    def done(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


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

"""Inputs shared by tests/test_crc32_host.py (CPU) and tests/test_crc32_device.py (GPU): the length-and-content grid of the CRC
tests, the inflate corpus with true trailer CRCs, and a copy of the fixture BAM with one damaged member that still inflates to
ISIZE bytes."""
import functools
import os
import random
import struct
import zlib

import numpy as np

import deflatewriter as D
import inflatecases as ic

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "data", "NA12878.target_loci.sorted.bam")

# the lengths straddle every chunk-count and alignment boundary of a 64-lane split
LENGTHS = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 127, 1023, 1024, 1025, 4095, 65279, 65535, 65536)


@functools.lru_cache(maxsize=None)
def grid():
    """(members, off): every length with all zero, all 0xFF, a counter and seeded random contents, and three members of 65 536
    bytes of which the second differs from the first in its last byte only, the third in its first byte only.  The members lie
    side by side, so their starts fall on every alignment."""
    rnd = random.Random(20261018)
    members = []
    for n in LENGTHS:
        members += [bytes(n), b"\xff" * n, bytes(k & 0xFF for k in range(n)), rnd.randbytes(n)]
    base = rnd.randbytes(65536)
    members += [base, base[:-1] + bytes([base[-1] ^ 0x40]), bytes([base[0] ^ 0x01]) + base[1:]]
    off = np.cumsum([0] + [len(m) for m in members]).astype(np.uint64)
    return tuple(members), off


def mixed(n=4096, seed=7):
    """(data, off): n members of mixed lengths in one buffer (most of them short, every grid length among them)"""
    rnd = random.Random(seed)
    lens = [LENGTHS[k % len(LENGTHS)] if k % 16 == 0 and LENGTHS[k % len(LENGTHS)] < 5000 else rnd.choice((0, 1, 7, 31, 100, 333, 1500, 4097)) + rnd.randrange(16)
            for k in range(n)]
    lens[n // 2], lens[n - 1] = 65536, 65279
    off = np.cumsum([0] + lens).astype(np.uint64)
    return rnd.randbytes(int(off[-1])), off


def with_true_crc(entries):
    """[(label, member)] of [(label, member, raw)] with the trailer's CRC32 set to zlib's"""
    out = []
    for label, m, raw in entries:
        payload, isize = ic.split_member(m)
        assert isize == len(raw)
        out.append((label, ic.member(payload, isize, zlib.crc32(raw))))
    return out


def flip_trailer_bit(m, bit):
    """the member with bit `bit` of its stored CRC32 flipped"""
    b = bytearray(m)
    b[len(b) - 8 + (bit >> 3)] ^= 1 << (bit & 7)
    return bytes(b)


def sized_member(rnd, n):
    raw = bytes(rnd.choices(b"ACGTN", k=n))                  # (compressible: 65 535 random bytes do not fit a member)
    return "size%d" % n, ic.member(ic.deflate(raw, 1), n, zlib.crc32(raw)), raw


def _members_of(data):
    out, at = [], 0
    while at + 18 <= len(data):
        size = (data[at + 16] | data[at + 17] << 8) + 1
        out.append((at, size))
        at += size
    return out


def _shift_bai(bai, behind, delta):
    """the index with every virtual offset whose block lies behind file offset `behind` moved by `delta` bytes"""
    out = bytearray(bai)
    move = lambda at: struct.pack_into("<Q", out, at, struct.unpack_from("<Q", bai, at)[0] + ((delta << 16) if (struct.unpack_from("<Q", bai, at)[0] >> 16) > behind else 0))
    at = 8
    for _ in range(struct.unpack_from("<i", bai, 4)[0]):
        n_bin = struct.unpack_from("<i", bai, at)[0]
        at += 4
        for _b in range(n_bin):
            n_chunk = struct.unpack_from("<i", bai, at + 4)[0]
            at += 8
            for _c in range(2 * n_chunk):       # (the pseudo-bin's second pair holds counts: far below any shifted offset's block)
                move(at)
                at += 8
        n_intv = struct.unpack_from("<i", bai, at)[0]
        at += 4
        for _i in range(n_intv):
            move(at)
            at += 8
    return bytes(out)


def damaged_fixture(dst, which=None):
    """A copy of the fixture at `dst` (with its index) in which one member is re-deflated as a stored block with ONE bit of its
    bytes flipped, under its old trailer: it still inflates to ISIZE bytes, and their CRC32 is not the stored one -- checked
    here with zlib alone.  The members behind it move; the index is rewritten to match.  Returns the member's file offset."""
    data = open(FIXTURE, "rb").read()
    members = _members_of(data)
    k = len(members) // 2 if which is None else which
    at, size = members[k]
    m = data[at:at + size]
    payload, isize = ic.split_member(m)
    raw = bytearray(zlib.decompress(payload, -15))
    assert len(raw) == isize and 1000 < isize <= 65505      # (the largest stored block a member holds)
    raw[isize // 2] ^= 0x10
    new = ic.member(D.write([D.stored(bytes(raw))]), isize)
    new = new[:-8] + m[-8:]                                   # the old trailer: the CRC32 of the undamaged bytes
    inflated = zlib.decompress(ic.split_member(new)[0], -15)
    stored = struct.unpack("<I", new[-8:-4])[0]
    assert len(inflated) == isize == struct.unpack("<I", new[-4:])[0]
    assert zlib.crc32(inflated) != stored and zlib.crc32(zlib.decompress(payload, -15)) == stored
    open(dst, "wb").write(data[:at] + new + data[at + size:])
    open(dst + ".bai", "wb").write(_shift_bai(open(FIXTURE + ".bai", "rb").read(), at, len(new) - size))
    return at

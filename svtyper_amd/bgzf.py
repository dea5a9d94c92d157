"""The BGZF layer under the BAM reader and under every writer: a reader by (compressed offset, in-block offset) addresses, a
writer member by member, and the close of a writer that held its whole output (bam.AlignmentFile with sort= / index=,
bgzf_out.BgzfTextWriter with sort= / index=).  Nothing here knows what a BAM record or a VCF line is."""
from __future__ import annotations

import os
import struct
import zlib
from collections import OrderedDict
from typing import List, Tuple


class BgzfReader:
    """Random access over a BGZF file through (compressed offset, in-block offset) addresses."""

    def __init__(self, path: str, cache_blocks: int = 64, verify: bool = False):
        self._f = open(path, "rb")
        self.verify = verify             # check every block's CRC32 where it is inflated (verify="crc32")
        self.members_verified = 0
        self._cache: "OrderedDict[int, Tuple[bytes, int]]" = OrderedDict()
        self._cache_blocks = cache_blocks
        self._coff = 0   # compressed offset of the current block
        self._uoff = 0   # offset inside the current block
        self._block = b""
        self._next = 0   # compressed offset of the next block

    def close(self):
        self._f.close()

    def _load(self, coff: int) -> bool:
        hit = self._cache.get(coff)
        if hit is not None:
            self._cache.move_to_end(coff)
            self._block, self._next = hit
            self._coff = coff
            return len(self._block) > 0 or self._next > coff
        self._f.seek(coff)
        hdr = self._f.read(18)
        if len(hdr) < 18:
            self._block, self._next, self._coff = b"", coff, coff
            return False
        if hdr[0] != 31 or hdr[1] != 139:
            raise IOError("not a BGZF block at offset %d" % coff)
        xlen = struct.unpack_from("<H", hdr, 10)[0]
        extra = hdr[12:18] + self._f.read(xlen - 6)
        bsize = None
        i = 0
        while i + 4 <= len(extra):
            si1, si2, slen = extra[i], extra[i + 1], struct.unpack_from("<H", extra, i + 2)[0]
            if si1 == 66 and si2 == 67:
                bsize = struct.unpack_from("<H", extra, i + 4)[0]
            i += 4 + slen
        if bsize is None:
            raise IOError("BGZF block without BC field")
        cdata_len = bsize - xlen - 19
        cdata = self._f.read(cdata_len)
        trailer = self._f.read(8)  # crc32 + isize
        data = zlib.decompress(cdata, -15) if cdata_len > 0 else b""
        if self.verify:
            stored = struct.unpack_from("<I", trailer, 0)[0] if len(trailer) >= 4 else None
            computed = zlib.crc32(data) & 0xFFFFFFFF
            self.members_verified += 1
            if stored != computed:
                raise IOError("BGZF block at offset %d: CRC32 mismatch (stored 0x%08x, computed 0x%08x)" % (coff, stored or 0, computed))
        nxt = coff + bsize + 1
        self._cache[coff] = (data, nxt)
        if len(self._cache) > self._cache_blocks:
            self._cache.popitem(last=False)
        self._block, self._next, self._coff = data, nxt, coff
        return True

    def seek(self, voffset: int):
        coff, uoff = voffset >> 16, voffset & 0xFFFF
        self._load(coff)
        self._uoff = uoff

    def tell(self) -> int:
        if self._uoff >= len(self._block) and self._block:
            return self._next << 16
        return (self._coff << 16) | self._uoff

    def read(self, n: int) -> bytes:
        out = []
        need = n
        while need > 0:
            avail = len(self._block) - self._uoff
            if avail <= 0:
                if not self._load(self._next):
                    break
                self._uoff = 0
                if not self._block:
                    # empty block (EOF marker) -- try the next one
                    if self._next == self._coff:
                        break
                    continue
                continue
            take = min(avail, need)
            out.append(self._block[self._uoff:self._uoff + take])
            self._uoff += take
            need -= take
        return b"".join(out)


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # the empty last member (SAM spec 4.1.2)
PAYLOAD = 0xff00            # bytes of payload per member, htslib's block size: with its header a stored member stays within 64 KiB


DEFLATE_CHOICES = ("zlib", "host", "device")
HUFFMAN_CHOICES = ("fixed", "dynamic")
_BGZF_BATCH = 256           # finished payloads handed to svt_bgzf_deflate_host / _device in one call


def check_deflate(deflate) -> str:
    if deflate not in DEFLATE_CHOICES:
        raise ValueError("deflate must be one of %s, not %r" % (", ".join(repr(c) for c in DEFLATE_CHOICES), deflate))
    return deflate


def check_huffman(huffman, deflate) -> str:
    """`huffman`: the block the library's own compressor writes; "dynamic" needs deflate="host" or "device" """
    if huffman not in HUFFMAN_CHOICES:
        raise ValueError("huffman must be one of %s, not %r" % (", ".join(repr(c) for c in HUFFMAN_CHOICES), huffman))
    if huffman == "dynamic" and deflate == "zlib":
        raise ValueError("huffman='dynamic' needs deflate='host' or deflate='device': with deflate='zlib' the blocks are zlib's own")
    return huffman


class BgzfWriter:
    """A BGZF file written member by member: at most 65 280 bytes of payload each, its CRC32 and ISIZE behind the deflate
    stream, the 28-byte empty member at the end.  `path_or_file`: a path, or a binary file object (closed by close()).

    deflate="zlib": every member goes through zlib at `level` as it is cut.  (Readable by any BGZF reader; not the bytes
    htslib's deflate would produce.)  deflate="host" / "device": finished payloads are collected and compressed _BGZF_BATCH at a
    time by one call of the library's own compressor (svtyper_amd/csrc/svt_deflate.h), on this thread or on GPU `device`; the
    library is imported with the first batch.  Where a payload is cut is decided before anybody compresses it, so the inflated
    stream and the member boundaries are the same for all three.  huffman="dynamic" (with "host" / "device" only; ValueError with
    "zlib"): every member that is shorter as a dynamic-Huffman block is written as one; the default "fixed" writes
    the bytes it always wrote."""

    def __init__(self, path_or_file, level: int = 6, deflate: str = "zlib", device: int = 0, huffman: str = "fixed"):
        self._deflate = check_deflate(deflate)
        self._huffman = check_huffman(huffman, self._deflate)
        self._f = path_or_file if hasattr(path_or_file, "write") else open(path_or_file, "wb")
        self._level = level
        self._device = device
        self._buf = bytearray()
        self._pending: List[bytes] = []      # (host / device) payloads that are cut and not yet compressed

    def write(self, data: bytes) -> None:
        self._buf += data
        while len(self._buf) >= PAYLOAD:
            self._member(bytes(self._buf[:PAYLOAD]))
            del self._buf[:PAYLOAD]

    def write_record(self, data: bytes) -> None:
        """`data` kept inside one member where it fits one"""
        if self._buf and len(self._buf) + len(data) > PAYLOAD:
            self.flush()
        self.write(data)

    def flush(self) -> None:
        """what is buffered becomes a member of its own (with host / device: once its batch is compressed -- drain())"""
        if self._buf:
            self._member(bytes(self._buf))
            del self._buf[:]

    def drain(self) -> None:
        """(host / device) the payloads cut so far compressed and written"""
        if not self._pending:
            return
        from . import native_reads
        assert native_reads.DEFLATE_MAX_PAYLOAD == PAYLOAD      # (the C header's dfl::kMaxPayload, mirrored there)
        members, _off = native_reads.bgzf_deflate(self._pending, device=self._device if self._deflate == "device" else None,
                                                  huffman=self._huffman)
        del self._pending[:]
        self._f.write(members.tobytes())

    def _member(self, payload: bytes) -> None:
        if self._deflate != "zlib":
            self._pending.append(payload)
            if len(self._pending) >= _BGZF_BATCH:
                self.drain()
            return
        for level in (self._level, 0):      # (level 0 = stored: payload + 5 bytes per deflate block, always within a member)
            z = zlib.compressobj(level, zlib.DEFLATED, -15)
            cdata = z.compress(payload) + z.flush()
            if len(cdata) + 26 <= 0x10000:
                break
        self._f.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(cdata) + 25) + cdata
                      + struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))

    def close(self) -> None:
        if self._f is not None:
            self.flush()
            self.drain()
            self._f.write(BGZF_EOF)
            self._f.close()
            self._f = None


class _MemberLog:
    """a binary file that notes where every BGZF member written to it begins (each write is whole members)"""

    def __init__(self, f):
        self._f = f
        self.offsets = [0]
        self.starts = [0]       # where each member's payload begins in the inflated stream (its ISIZE says how long it is)

    def write(self, data) -> int:
        at, n, base = 0, len(data), self.offsets[-1]
        while at < n and data[at:at + 28] != BGZF_EOF:
            at += struct.unpack_from("<H", data, at + 16)[0] + 1
            self.offsets.append(base + at)
            self.starts.append(self.starts[-1] + struct.unpack_from("<I", data, at - 4)[0])
        return self._f.write(data)

    def flush(self):
        self._f.flush()

    def close(self):
        self._f.close()


def close_held(w: BgzfWriter, index_path, members, fold, order_error, write_index, stale=()) -> None:
    """The close of a writer that held its whole output until now, over its BgzfWriter `w` (nothing written to it yet): the
    members are logged as they are written, an index of an earlier file is not left beside this one, the data file is complete
    and closed whatever happens, and only then is the index folded and written, or refused.  The writer supplies
        members(w) -> held            writes every member through `w` (or whole members to w._f); raises where the order is refused
        fold(held, log) -> (index bytes, bad, kind)     from the _MemberLog's offsets / starts; None: no index was asked for
        order_error(held, bad, kind)  the exception for a fold that stopped at `bad`;  write_index(index_path, index bytes)
    `stale`: the default index paths of the output in either format (X.bai and X.csi; X.tbi and X.csi) -- an index of an earlier
    file under one of them would be read in place of the one written now (the project's own readers prefer a .bai)."""
    log = w._f = _MemberLog(w._f)
    for path in ((index_path,) if index_path is not None else ()) + tuple(stale):
        if os.path.exists(path):
            os.remove(path)
    try:
        held = members(w)
    finally:
        w.close()
    if fold is None:
        return
    index, bad, kind = fold(held, log)
    if bad:
        raise order_error(held, bad, kind)
    write_index(index_path, index)

"""CRAM 3.0 reader with the `AlignmentFile` surface bam.py lists for reading.

Written from the published format (CRAM format specification 3.0): the file definition, containers and blocks with their
CRC32s, the SAM-header container, the compression header, slice headers (several slices per container, multi-reference slices),
the EOF container and the `.crai` index.  It was checked against an independent writer made from the same text
(tests/cramwriter.py); it has never seen a file written by htslib.

What is Python here is the walk over containers and blocks and the index; the block methods raw, gzip, bzip2 and lzma go
through `zlib`, `bz2` and `lzma`.  What is native: rANS 4x8 (block method 4) -- `rans_decode`, one batch call for all the blocks
of a fetch or of up to 64 MiB of containers, by the host twin or the device twin of svt_rans.h (`codec="host" | "device"`) --
and the slice decoder (svt_cram.h: `decode_slice`), which turns a slice's data series into BAM record bytes.  Records are
`bam.AlignedSegment`s over those bytes, so everything behind the reader (fragments, `record_of`, `RecordSink`, the sorted `-w`
writer) takes them as it takes a BAM's.

SVTyper never looks at bases or qualities (bam.py's docstring): SEQ is `N` x read length, QUAL 0xFF x read length, `bin` is
reg2bin of the record's extent, and no reference FASTA is read (`-T` is accepted and not needed).

Refused with one CramError naming the file and what was met: major version 2; the block methods of minor version 1 (5 to 8:
`samtools view -O cram,version=3.0` writes a file this reader takes); the GOLOMB and GOLOMB_RICE encodings; a truncated
container; an encoding that reads past its block; with `verify`, a CRC32 that differs.  Nothing is repaired.
"""
from __future__ import annotations

import ctypes as C
import gzip
import mmap
import os
import struct
import zlib
from collections import OrderedDict
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import hip
from .bam import AlignedSegment, AlignmentFile

CODEC_CHOICES = ("host", "device")
BATCH_BYTES = 64 << 20          # containers handed to one rANS batch call by the whole-file walk
SLICE_CACHE = 8                 # decoded slices kept (the two fetches of a breakpoint often hit the same slice)
RANS_REASONS = {1: "its header does not fit the block", 2: "its frequency table is malformed or does not sum to 4096",
                3: "its input runs out", 4: "a state points at no symbol", 5: "order 1 with nothing to decode"}
_EOF_START = 4542278            # "EOF" as the start position of the last container


class CramError(IOError):
    """a CRAM file that is refused: the message names the file and what was met"""


def check_codec(codec: str) -> str:
    if codec not in CODEC_CHOICES:
        raise ValueError("cram_codec must be 'host' or 'device'")
    return codec


def is_cram(path: str) -> bool:
    """what a file is, its magic says"""
    try:
        with open(path, "rb") as f:
            return f.read(4) == b"CRAM"
    except OSError:
        return False


# ------------------------------------------------------------------------------------------ native calls
class _SliceInfo(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("bytes", C.c_uint64)]


class RansTimes(C.Structure):
    _fields_ = [("upload_s", C.c_double), ("order0_kernel_s", C.c_double), ("order1_kernel_s", C.c_double), ("download_s", C.c_double),
                ("total_s", C.c_double)]


_declared = False


def _lib():
    global _declared
    L = hip.load()
    if not _declared:
        if not hasattr(L, "svt_rans_decode_host"):
            raise hip.SvtyperHipError("libsvtyper_hip.so was built before the CRAM reader: rebuild it (svt_rans_decode_host is missing)")
        batch = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.svt_rans_decode_host.restype = C.c_int
        L.svt_rans_decode_host.argtypes = batch
        L.svt_rans_decode_device.restype = C.c_int
        L.svt_rans_decode_device.argtypes = batch + [C.c_int]
        L.svt_rans_last_times.restype = C.c_int
        L.svt_rans_last_times.argtypes = [C.POINTER(RansTimes)]
        L.svt_cram_decode_slice.restype = C.c_int
        L.svt_cram_decode_slice.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_char_p, C.c_uint32, C.c_int32, C.POINTER(_SliceInfo)]
        L.svt_cram_take.restype = C.c_int
        L.svt_cram_take.argtypes = [C.c_void_p, C.c_void_p]
        _declared = True
    return L


def rans_decode(blocks, out_sizes, codec: str = "host", device: int = 0, guard: int = 0, fill: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """svt_rans_decode_host / svt_rans_decode_device over the rANS 4x8 blocks `blocks` (each: order byte, compressed size,
    uncompressed size, payload), block k decoding to out_sizes[k] bytes.  -> (out uint8, out_off uint64 [n], status uint32 [n]):
    block k's bytes are out[out_off[k] : out_off[k] + out_sizes[k]], zeros where status[k] (a RANS_REASONS key) is not 0.  `guard`:
    that many bytes of value `fill` in front of, between and behind the outputs, which a correct decoder leaves alone."""
    L = _lib()
    check_codec(codec)
    n = len(blocks)
    lens = np.fromiter((len(b) for b in blocks), np.uint64, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(bytes(b) for b in blocks), np.uint8) if int(off[-1]) else np.zeros(1, np.uint8)
    sizes = np.ascontiguousarray(out_sizes, np.uint64)
    if sizes.shape[0] != n:
        raise ValueError("out_sizes holds one entry per block")
    out_off = np.zeros(n, np.uint64)
    if n:
        out_off[:] = np.cumsum(sizes + np.uint64(guard)) - sizes
    out_len = int(sizes.sum()) + guard * (n + 1)
    out = np.full(max(out_len, 1), fill, np.uint8)
    status = np.zeros(max(n, 1), np.uint32)
    args = [data.ctypes.data, int(off[-1]), off.ctypes.data, n, out_off.ctypes.data, sizes.ctypes.data, out.ctypes.data, out_len, status.ctypes.data]
    if codec == "device":
        hip._check(L.svt_rans_decode_device(*args, int(device)))
    else:
        hip._check(L.svt_rans_decode_host(*args))
    return out[:out_len], out_off, status[:n]


def rans_last_times() -> dict:
    """the calling thread's most recent device batch: copies and kernels by HIP events, the whole call on the host's clock"""
    t = RansTimes()
    hip._check(_lib().svt_rans_last_times(C.byref(t)))
    return {name: getattr(t, name) for name, _ in RansTimes._fields_}


def decode_slice(comp_header: bytes, slice_header: bytes, blocks: List[Tuple[int, bool, bytes]], rg_ids: List[str], n_ref: int) -> Tuple[bytes, np.ndarray]:
    """svt_cram_decode_slice + svt_cram_take: the slice's records as BAM record bytes (block_size first) and their n + 1 offsets.
    `blocks`: (content id, is the core block, content) of the slice's blocks behind its header.  Raises hip.SvtyperHipError with
    what was met for a slice that is refused."""
    L = _lib()
    n = len(blocks)
    lens = np.fromiter((len(b[2]) for b in blocks), np.uint64, n)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    data = b"".join(bytes(b[2]) for b in blocks) or b"\0"
    ids = np.array([b[0] for b in blocks] or [0], np.int32)
    core = np.array([1 if b[1] else 0 for b in blocks] or [0], np.uint8)
    rg = b"".join(s.encode("ascii") + b"\0" for s in rg_ids) or b"\0"
    info = _SliceInfo()
    comp, sl = bytes(comp_header), bytes(slice_header)
    hip._check(L.svt_cram_decode_slice(comp, len(comp), sl, len(sl), data, off.ctypes.data, ids.ctypes.data, core.ctypes.data, n, rg, len(rg_ids),
                                       int(n_ref), C.byref(info)))
    records = np.zeros(max(int(info.bytes), 1), np.uint8)
    rec_off = np.zeros(int(info.n_records) + 1, np.uint64)
    hip._check(L.svt_cram_take(records.ctypes.data, rec_off.ctypes.data))
    return records[:int(info.bytes)].tobytes(), rec_off


# ------------------------------------------------------------------------------------------ the container layer
class _Cursor:
    """bytes read in order; running out raises struct.error, which the callers turn into `truncated`"""

    def __init__(self, data, at=0, end=None):
        self.data, self.at, self.end = data, at, len(data) if end is None else end

    def u8(self) -> int:
        if self.at >= self.end:
            raise struct.error("out of bytes")
        self.at += 1
        return self.data[self.at - 1]

    def take(self, n: int):
        if n < 0 or self.at + n > self.end:
            raise struct.error("out of bytes")
        self.at += n
        return self.data[self.at - n:self.at]

    def i32(self) -> int:
        return struct.unpack("<i", self.take(4))[0]

    def u32(self) -> int:
        return struct.unpack("<I", self.take(4))[0]

    def itf8(self) -> int:
        b = self.u8()
        if b < 0x80:
            v = b
        elif b < 0xC0:
            v = (b & 0x3F) << 8 | self.u8()
        elif b < 0xE0:
            v = (b & 0x1F) << 16 | self.u8() << 8 | self.u8()
        elif b < 0xF0:
            v = (b & 0x0F) << 24 | self.u8() << 16 | self.u8() << 8 | self.u8()
        else:
            v = (b & 0x0F) << 28 | self.u8() << 20 | self.u8() << 12 | self.u8() << 4 | (self.u8() & 0x0F)
        return v - (1 << 32) if v & (1 << 31) else v

    def ltf8(self) -> int:
        b = self.u8()
        extra = 0
        while extra < 8 and b & (0x80 >> extra):
            extra += 1
        v = b & (0xFF >> (extra + 1)) if extra < 7 else 0
        for _ in range(extra):
            v = v << 8 | self.u8()
        return v - (1 << 64) if v & (1 << 63) else v


class _Block:
    __slots__ = ("method", "ctype", "cid", "raw_size", "data", "at", "content")

    def __init__(self, method, ctype, cid, raw_size, data, at):
        self.method, self.ctype, self.cid, self.raw_size, self.data, self.at = method, ctype, cid, raw_size, data, at
        self.content = None          # the block with its method undone


class _Container:
    __slots__ = ("at", "length", "ref", "start", "span", "n_records", "counter", "n_blocks", "landmarks", "data_at", "end")


class CramFile:
    """CRAM 3.0 file opened for reading, with its .crai index where fetch(contig, ...) needs it."""

    def __init__(self, path: str, mode: str = "rc", verify: bool = False, codec: str = "host", device: int = 0, **kwargs):
        if mode not in ("rc", "rb", "r"):
            raise NotImplementedError("CRAM output is not written")
        self.filename = path
        self.verify = bool(verify)
        self.codec, self.device = check_codec(codec), int(device)
        self.blocks_verified = 0
        self._f = open(path, "rb")
        size = os.fstat(self._f.fileno()).st_size
        self._map = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ) if size else b""
        self._size = size
        m = self._map
        if size < 26 or m[:4] != b"CRAM":
            raise CramError("%s is not a CRAM file" % path)
        self.version = (m[4], m[5])
        if m[4] == 2:
            raise CramError("%s: CRAM major version 2 is not read (this reader takes CRAM 3.0)" % path)
        if m[4] != 3:
            raise CramError("%s: CRAM major version %d is not read (this reader takes CRAM 3.0)" % (path, m[4]))
        head = self._container(26)
        if head is None:
            raise CramError("%s: truncated container at offset 26 (the SAM header)" % path)
        blocks = self._blocks(head)
        if not blocks or blocks[0].ctype != 0:
            raise CramError("%s: the first container does not hold the SAM header" % path)
        self._undo(blocks[:1])
        text = bytes(blocks[0].content)
        if len(text) < 4 or struct.unpack_from("<i", text, 0)[0] > len(text) - 4 or struct.unpack_from("<i", text, 0)[0] < 0:
            raise CramError("%s: the SAM header block is shorter than it says" % path)
        self.text = text[4:4 + struct.unpack_from("<i", text, 0)[0]].split(b"\0", 1)[0].decode("ascii", "replace")
        self.header = AlignmentFile._parse_header(self.text)
        refs = [(sq.get("SN", ""), int(sq.get("LN", 0))) for sq in self.header.get("SQ", [])]
        self.references = tuple(r[0] for r in refs)
        self.lengths = tuple(r[1] for r in refs)
        self._tid = {r: i for i, r in enumerate(self.references)}
        self._rg_ids = [rg.get("ID", "") for rg in self.header.get("RG", [])]
        # the header as a BAM has it: what a file opened 'wb' with this one as template starts with
        raw_text = self.text.encode("ascii", "replace")
        self._header_bytes = (b"BAM\1" + struct.pack("<i", len(raw_text)) + raw_text + struct.pack("<i", len(refs))
                              + b"".join(struct.pack("<i", len(n) + 1) + n.encode("ascii") + b"\0" + struct.pack("<i", l) for n, l in refs))
        self._first = head.end
        self._crai = None
        self._cache: "OrderedDict[Tuple[int, int], Tuple[bytes, np.ndarray]]" = OrderedDict()
        self._counts = None

    # ---- containers and blocks
    def _container(self, at: int) -> Optional[_Container]:
        """the container header at `at`; None at the end of the file.  CramError for one that is cut short."""
        if at >= self._size:
            return None
        m = self._map
        c = _Container()
        try:
            cur = _Cursor(m, at, self._size)
            c.at = at
            c.length = cur.i32()
            c.ref, c.start, c.span, c.n_records = cur.itf8(), cur.itf8(), cur.itf8(), cur.itf8()
            c.counter, _bases = cur.ltf8(), cur.ltf8()
            c.n_blocks = cur.itf8()
            c.landmarks = [cur.itf8() for _ in range(cur.itf8())]
            stored = cur.u32()
        except struct.error:
            raise CramError("%s: truncated container at offset %d (its header runs out of the file)" % (self.filename, at))
        c.data_at = cur.at
        c.end = c.data_at + c.length
        if c.length < 0 or c.end > self._size:
            raise CramError("%s: truncated container at offset %d (%d bytes of blocks, %d left in the file)"
                            % (self.filename, at, c.length, self._size - c.data_at))
        if self.verify and zlib.crc32(m[at:c.data_at - 4]) & 0xFFFFFFFF != stored:
            raise CramError("%s: container at offset %d: CRC32 mismatch in its header" % (self.filename, at))
        return c

    @staticmethod
    def _is_eof(c: _Container) -> bool:
        return c.ref == -1 and c.start == _EOF_START and c.n_records == 0

    def _blocks(self, c: _Container, at: Optional[int] = None, count: Optional[int] = None) -> List[_Block]:
        """the blocks of container `c` (from offset `at`, `count` of them), not yet decompressed"""
        m = self._map
        cur = _Cursor(m, c.data_at if at is None else at, c.end)
        out = []
        try:
            for _ in range(c.n_blocks if count is None else count):
                at0 = cur.at
                method, ctype = cur.u8(), cur.u8()
                cid, csize, rsize = cur.itf8(), cur.itf8(), cur.itf8()
                data = cur.take(csize)
                stored = cur.u32()
                if self.verify:
                    if zlib.crc32(m[at0:cur.at - 4]) & 0xFFFFFFFF != stored:
                        raise CramError("%s: block at offset %d: CRC32 mismatch" % (self.filename, at0))
                    self.blocks_verified += 1
                out.append(_Block(method, ctype, cid, rsize, data, at0))
        except struct.error:
            raise CramError("%s: truncated container at offset %d (a block runs out of it)" % (self.filename, c.at))
        return out

    def _undo(self, blocks: List[_Block]) -> None:
        """the block methods of `blocks` undone: the rANS blocks among them in one batch call"""
        rans = []
        for b in blocks:
            if b.content is not None:
                continue
            try:
                if b.method == 0:
                    b.content = b.data
                elif b.method == 1:
                    b.content = zlib.decompress(b.data, 31)
                elif b.method == 2:
                    import bz2
                    b.content = bz2.decompress(b.data)
                elif b.method == 3:
                    import lzma
                    b.content = lzma.decompress(b.data)
                elif b.method == 4:
                    rans.append(b)
                    continue
                elif 5 <= b.method <= 8:
                    raise CramError("%s: block at offset %d uses block method %d, one of CRAM 3.1's codecs, which are not read: "
                                    "`samtools view -O cram,version=3.0` writes a file this reader takes" % (self.filename, b.at, b.method))
                else:
                    raise CramError("%s: block at offset %d: unknown block method %d" % (self.filename, b.at, b.method))
            except (zlib.error, OSError, ValueError, EOFError) as e:
                if isinstance(e, CramError):
                    raise
                raise CramError("%s: block at offset %d does not decompress (%s)" % (self.filename, b.at, e))
            if len(b.content) != b.raw_size:
                raise CramError("%s: block at offset %d decompresses to %d bytes, not the %d it says" % (self.filename, b.at, len(b.content), b.raw_size))
        if rans:
            out, out_off, status = rans_decode([b.data for b in rans], [b.raw_size for b in rans], self.codec, self.device)
            for b, o, st in zip(rans, out_off.tolist(), status.tolist()):
                if st:
                    raise CramError("%s: block at offset %d: the rANS block is refused (%s)" % (self.filename, b.at, RANS_REASONS.get(st, st)))
                b.content = out[o:o + b.raw_size].tobytes()

    def _slices(self, c: _Container, want=None) -> List[Tuple[Tuple[int, int], _Block, _Block, List[_Block]]]:
        """the slices of `c` (those whose landmark is in `want`) as (cache key, compression header block, slice header block,
        the slice's blocks); nothing decompressed but the two headers"""
        blocks = self._blocks(c)
        if not blocks or blocks[0].ctype != 1:
            raise CramError("%s: container at offset %d does not begin with a compression header" % (self.filename, c.at))
        out, cur = [], None
        for b in blocks[1:]:
            if b.ctype == 2:
                cur = ((c.at, b.at - c.data_at), blocks[0], b, [])
                out.append(cur)
            elif cur is None:
                raise CramError("%s: container at offset %d: a data block in front of the first slice header" % (self.filename, c.at))
            else:
                cur[3].append(b)
        if want is not None:
            out = [s for s in out if s[0][1] in want]
        return out

    def _decode(self, slices) -> List[Tuple[bytes, np.ndarray]]:
        """the decoded slices (records, offsets) of `slices` (_slices entries), through the cache; their blocks' methods are
        undone in one batch"""
        todo = [s for s in slices if s[0] not in self._cache]
        pending = []
        for _key, comp, sl, blocks in todo:
            pending.extend([comp, sl] + blocks)
        self._undo(pending)
        fresh = {}
        for key, comp, sl, blocks in todo:
            try:
                fresh[key] = decode_slice(comp.content, sl.content, [(b.cid, b.ctype == 5, b.content) for b in blocks], self._rg_ids, len(self.references))
            except hip.SvtyperHipError as e:
                raise CramError("%s: slice at offset %d: %s" % (self.filename, sl.at, str(e).split(": ", 1)[-1]))
        out = []
        for s in slices:
            got = fresh.get(s[0])
            if got is None:
                got = self._cache[s[0]]
                self._cache.move_to_end(s[0])
            out.append(got)
        for key, got in fresh.items():
            self._cache[key] = got
            while len(self._cache) > SLICE_CACHE:
                self._cache.popitem(last=False)
        return out

    def _records(self, data: bytes, rec_off: np.ndarray) -> Iterator[AlignedSegment]:
        off = rec_off.tolist()
        for a, b in zip(off[:-1], off[1:]):
            yield AlignedSegment(self, data[a + 4:b])

    def _walk(self) -> Iterator[AlignedSegment]:
        """every record of the file in file order; the rANS blocks of up to BATCH_BYTES of containers go to one batch call"""
        at = self._first
        while True:
            batch, taken = [], 0
            while taken < BATCH_BYTES:
                c = self._container(at)
                if c is None or self._is_eof(c):
                    at = None
                    break
                batch.extend(self._slices(c))
                taken += c.end - c.at
                at = c.end
            # (the cache is for fetches: a walk does not go through it)
            pending = []
            for _key, comp, sl, blocks in batch:
                pending.extend([comp, sl] + blocks)
            self._undo(pending)
            for _key, comp, sl, blocks in batch:
                try:
                    data, rec_off = decode_slice(comp.content, sl.content, [(b.cid, b.ctype == 5, b.content) for b in blocks], self._rg_ids,
                                                 len(self.references))
                except hip.SvtyperHipError as e:
                    raise CramError("%s: slice at offset %d: %s" % (self.filename, sl.at, str(e).split(": ", 1)[-1]))
                yield from self._records(data, rec_off)
            if at is None:
                return

    # ---- the index
    def _load_crai(self) -> None:
        stem = os.path.splitext(self.filename)[0]
        names = (self.filename + ".crai", stem + ".crai")
        for cand in names:
            if os.path.exists(cand):
                break
        else:
            raise ValueError("fetch called on a CRAM without index: neither %s nor %s is there" % names)
        try:
            with gzip.open(cand, "rb") as f:
                text = f.read().decode("ascii")
            entries = []
            for line in text.splitlines():
                if line.strip():
                    ref, start, span, coff, soff, size = (int(x) for x in line.split("\t")[:6])
                    entries.append((ref, start, span, coff, soff, size))
        except (OSError, EOFError, ValueError, zlib.error) as e:
            raise CramError("%s is not a .crai index (%s)" % (cand, e))
        self._crai = entries

    # ---- the AlignmentFile surface
    def gettid(self, reference: str) -> int:
        return self._tid.get(reference, -1)

    def get_reference_name(self, tid: int) -> str:
        return self.references[tid]

    def index_info(self) -> Optional[dict]:
        return None if self._crai is None else {"kind": "crai"}

    def close(self):
        self._cache.clear()
        if self._size:
            self._map.close()
        self._f.close()

    def _count_all(self) -> Tuple[int, int]:
        if self._counts is None:
            mapped = unmapped = 0
            for r in self._walk():
                if r.flag & 0x4:
                    unmapped += 1
                else:
                    mapped += 1
            self._counts = (mapped, unmapped)
        return self._counts

    @property
    def mapped(self) -> int:
        """(a .crai holds no counts: one pass over the file at first use)"""
        return self._count_all()[0]

    @property
    def unmapped(self) -> int:
        return self._count_all()[1]

    def fetch(self, contig: Optional[str] = None, start=None, stop=None, **kwargs) -> Iterator[AlignedSegment]:
        """Reads overlapping [start, stop) in file order; all placed reads when contig is None (as bam.AlignmentFile.fetch)."""
        reference = kwargs.get("reference", contig)
        if "end" in kwargs and stop is None:
            stop = kwargs["end"]
        if reference is None:
            for r in self._walk():
                if r.reference_id < 0:
                    return
                yield r
            return
        tid = self.gettid(reference)
        if tid < 0:
            raise ValueError("invalid contig `%s`" % reference)
        beg = 0 if start is None else max(0, int(start))
        end = self.lengths[tid] if stop is None else int(stop)
        if end <= beg:
            return
        if self._crai is None:
            self._load_crai()
        by_container: "OrderedDict[int, set]" = OrderedDict()
        for ref, s1, span, coff, soff, _size in self._crai:
            # (start is 1-based; a slice of span 0 is taken as one base)
            if ref == tid and s1 - 1 < end and s1 - 1 + max(span, 1) > beg:
                by_container.setdefault(coff, set()).add(soff)
        for coff in sorted(by_container):
            c = self._container(coff)
            if c is None:
                raise CramError("%s: the index names a container at offset %d, behind the end of the file" % (self.filename, coff))
            for data, rec_off in self._decode(self._slices(c, by_container[coff])):
                for r in self._records(data, rec_off):
                    if r.reference_id != tid or r.reference_start >= end:
                        continue
                    rend = r.reference_end
                    if rend is None or rend <= r.reference_start:
                        rend = r.reference_start + 1
                    if rend > beg:
                        yield r

    def count(self, contig=None, start=None, stop=None, read_callback="nofilter", **kwargs) -> int:
        n = 0
        for r in self.fetch(contig, start, stop, **kwargs):
            if read_callback == "all":
                if r.flag & (0x4 | 0x100 | 0x200 | 0x400):
                    continue
            n += 1
        return n

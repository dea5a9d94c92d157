"""Minimal BGZF / BAM / BAI / CSI reader with the slice of the pysam API the SVTyper path relies on.

pysam (htslib) is what the reference uses (svtyper/classic.py:126-129, parsers.py:480-558); it
is not available in this image and cannot be installed, so the host side ships its own reader.
Only what SURVEY.md section 3.5 lists is implemented:

    AlignmentFile(path, 'rb'): filename, header['RG'], references, lengths, gettid(), fetch(),
                               count(read_callback='all'), mapped, unmapped, close()
    AlignmentFile(path, 'wb', template=...): write(read), close() -- the evidence dump of `svtyper -w`: the template's
                               header, every record without its sequence, BGZF through zlib (or deflate="host" / "device")
    AlignedSegment: query_name, flag and its bits, reference_id/name, reference_start (= pos),
                    reference_end, mapping_quality, template_length, cigar (= cigartuples),
                    has_tag/get_tag/set_tag, get_overlap, query_length, query_alignment_length,
                    infer_query_length, query_sequence = None (the only value it takes)

CRAM 3.0 is read by cram.py (`CramFile`: the same reading surface, its records AlignedSegments over BAM record bytes the native
slice decoder makes).  SVTyper never looks at bases or qualities, so those records carry SEQ as `N` x read length, QUAL as 0xFF
x read length and `bin` as reg2bin of their extent, and no reference FASTA is needed.
If a real pysam is importable, `open_alignment_file` prefers it.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Dict, Iterator, List, Optional, Tuple

# the BGZF layer (bgzf.py), under the names it always had here
from .bgzf import BGZF_EOF, DEFLATE_CHOICES, HUFFMAN_CHOICES, BgzfReader, BgzfWriter, check_deflate, check_huffman, close_held  # noqa: F401

# CIGAR op codes: M I D N S H P = X
_CONSUMES_REF = (True, False, True, True, False, False, False, True, True)
_ALIGNED = (True, False, False, False, False, False, False, True, True)  # M = X


_TAG_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def _without_tag(b: bytes, key: str) -> bytes:
    """the tag area `b` without the fields named `key`"""
    name = key.encode("ascii")
    out = []
    i, n = 0, len(b)
    while i + 3 <= n:
        t = chr(b[i + 2])
        j = i + 3
        if t in _TAG_SIZE:
            j += _TAG_SIZE[t]
        elif t in "ZH":
            j = b.index(b"\0", j) + 1
        elif t == "B":
            j += 5 + struct.unpack_from("<I", b, j + 1)[0] * _TAG_SIZE[chr(b[j])]
        else:
            raise ValueError("unknown BAM tag type %r" % t)
        if b[i:i + 2] != name:
            out.append(b[i:j])
        i = j
    return b"".join(out)


def _encode_tag(key: str, value) -> bytes:
    name = key.encode("ascii")
    if isinstance(value, str):
        if len(value) == 1:
            return name + b"A" + value.encode("ascii")
        return name + b"Z" + value.encode("ascii") + b"\0"
    if isinstance(value, float):
        return name + b"f" + struct.pack("<f", value)
    if isinstance(value, int):
        return name + b"i" + struct.pack("<i", value)
    raise TypeError("tag %s: a value of type %s is not written" % (key, type(value).__name__))


class AlignedSegment:
    """One BAM record; attribute names follow pysam."""

    __slots__ = ("_file", "query_name", "flag", "reference_id", "reference_start", "mapping_quality",
                 "next_reference_id", "next_reference_start", "template_length", "cigar", "query_length",
                 "_tagbytes", "_tags", "_ref_end", "_raw_seq", "_raw", "_set_tags")

    def __init__(self, afile, data: bytes):
        (ref_id, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, next_pos, tlen) = \
            struct.unpack_from("<iiBBHHHiiii", data, 0)
        self._file = afile
        self._raw = data                 # the record as it lies in the file (behind block_size): what AlignmentFile.write starts from
        self._set_tags = None            # the names set_tag was given, in the order of their last call
        self.reference_id = ref_id
        self.reference_start = pos
        self.mapping_quality = mapq
        self.flag = flag
        self.next_reference_id = next_ref
        self.next_reference_start = next_pos
        self.template_length = tlen
        off = 32
        self.query_name = data[off:off + l_read_name - 1].decode("ascii")
        off += l_read_name
        if n_cigar:
            raw = struct.unpack_from("<%dI" % n_cigar, data, off)
            self.cigar = [(c & 0xF, c >> 4) for c in raw]
        else:
            self.cigar = []
        off += 4 * n_cigar
        self.query_length = l_seq                      # pysam: l_seq of the record
        self._raw_seq = None
        off += (l_seq + 1) // 2 + l_seq
        self._tagbytes = data[off:]
        self._tags: Optional[Dict[str, object]] = None
        self._ref_end = None

    # ---- flag bits
    @property
    def is_paired(self): return bool(self.flag & 0x1)
    @property
    def is_proper_pair(self): return bool(self.flag & 0x2)
    @property
    def is_unmapped(self): return bool(self.flag & 0x4)
    @property
    def mate_is_unmapped(self): return bool(self.flag & 0x8)
    @property
    def is_reverse(self): return bool(self.flag & 0x10)
    @property
    def mate_is_reverse(self): return bool(self.flag & 0x20)
    @property
    def is_read1(self): return bool(self.flag & 0x40)
    @property
    def is_read2(self): return bool(self.flag & 0x80)
    @property
    def is_secondary(self): return bool(self.flag & 0x100)
    @property
    def is_qcfail(self): return bool(self.flag & 0x200)
    @property
    def is_duplicate(self): return bool(self.flag & 0x400)
    @property
    def is_supplementary(self): return bool(self.flag & 0x800)

    # ---- coordinates
    @property
    def pos(self):
        return self.reference_start

    @property
    def reference_name(self):
        return self._file.references[self.reference_id] if self.reference_id >= 0 else None

    @property
    def reference_end(self):
        """pos + sum of the reference-consuming CIGAR operations (None when there is no CIGAR)."""
        if self._ref_end is None:
            if not self.cigar:
                return None
            end = self.reference_start
            for op, n in self.cigar:
                if _CONSUMES_REF[op]:
                    end += n
            self._ref_end = end
        return self._ref_end

    @property
    def cigartuples(self):
        return self.cigar

    @property
    def query_alignment_length(self):
        return sum(n for op, n in self.cigar if op in (0, 1, 7, 8))

    def infer_query_length(self):
        return sum(n for op, n in self.cigar if op in (0, 1, 4, 7, 8))

    def get_overlap(self, start: int, end: int) -> int:
        """Number of M/=/X-aligned reference bases inside [start, end)."""
        ov = 0
        p = self.reference_start
        for op, n in self.cigar:
            if _ALIGNED[op]:
                lo = p if p > start else start
                hi = p + n if p + n < end else end
                if hi > lo:
                    ov += hi - lo
            if _CONSUMES_REF[op]:
                p += n
        return ov

    # ---- tags
    _STRING_TAGS = ("RG", "SA")

    def _parse_tags(self):
        tags: Dict[str, object] = {}
        b = self._tagbytes
        i, n = 0, len(b)
        while i + 3 <= n:
            key = b[i:i + 2].decode("ascii")
            t = chr(b[i + 2])
            i += 3
            if t == "A":
                val = chr(b[i]); i += 1
            elif t == "c":
                val = struct.unpack_from("<b", b, i)[0]; i += 1
            elif t == "C":
                val = b[i]; i += 1
            elif t == "s":
                val = struct.unpack_from("<h", b, i)[0]; i += 2
            elif t == "S":
                val = struct.unpack_from("<H", b, i)[0]; i += 2
            elif t == "i":
                val = struct.unpack_from("<i", b, i)[0]; i += 4
            elif t == "I":
                val = struct.unpack_from("<I", b, i)[0]; i += 4
            elif t == "f":
                val = struct.unpack_from("<f", b, i)[0]; i += 4
            elif t in "ZH":
                j = b.index(b"\0", i)
                val = b[i:j].decode("ascii"); i = j + 1
            elif t == "B":
                sub = chr(b[i]); cnt = struct.unpack_from("<I", b, i + 1)[0]; i += 5
                fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
                sz = struct.calcsize(fmt)
                val = list(struct.unpack_from("<%d%s" % (cnt, fmt), b, i)); i += cnt * sz
            else:
                raise ValueError("unknown BAM tag type %r" % t)
            # A record holds a tag name once (SAM 1.5) and RG and SA are strings.  Where a record departs from that the native
            # reader's rule holds (rr::walk_tags): the first value of a name, and under RG and SA only a value of type Z.
            if key not in tags and (t == "Z" or key not in self._STRING_TAGS):
                tags[key] = val
        self._tags = tags

    def has_tag(self, key: str) -> bool:
        if self._tags is None:
            self._parse_tags()
        return key in self._tags

    def get_tag(self, key: str):
        if self._tags is None:
            self._parse_tags()
        return self._tags[key]  # KeyError like pysam

    def set_tag(self, key: str, value, value_type=None):
        if self._tags is None:
            self._parse_tags()
        self._tags[key] = value
        if self._set_tags is None:
            self._set_tags = []
        elif key in self._set_tags:
            self._set_tags.remove(key)
        self._set_tags.append(key)

    @property
    def query_sequence(self):
        """the reader never decodes the sequence; svtyper/utils.py:14 sets it to None before a read is written"""
        return None

    @query_sequence.setter
    def query_sequence(self, value):
        if value is not None:
            raise NotImplementedError("query_sequence can only be set to None (the sequence is dropped on write)")

    def __repr__(self):
        return "<AlignedSegment %s flag=%d %s:%d mapq=%d>" % (
            self.query_name, self.flag, self.reference_name, self.reference_start, self.mapping_quality)


def _reg2bins(beg: int, end: int, min_shift: int = 14, depth: int = 5) -> List[int]:
    """Bins overlapping [beg, end) in a scheme of `depth` levels over leaves of 2^min_shift positions (SAM spec 5.3, CSIv1):
    level l starts at bin (8^l - 1) / 7 and shifts by min_shift + 3 (depth - l).  (14, 5) is the BAI's UCSC scheme."""
    end -= 1
    bins: List[int] = []
    for l in range(depth + 1):
        shift, off = min_shift + 3 * (depth - l), ((1 << (3 * l)) - 1) // 7
        bins.extend(range(off + (beg >> shift), off + (end >> shift) + 1))
    return bins


def _pseudo_bin(depth: int) -> int:
    """the bin number that carries a reference's mapped / unmapped counts: 37450 at depth 5"""
    return ((1 << (3 * (depth + 1))) - 1) // 7 + 1


class BamOrderError(ValueError):
    """the records cannot be sorted or indexed as they are: `record` is the 1-based number of the record in the way, among
    those handed to write() / write_raw()"""

    def __init__(self, message: str, record: int):
        super().__init__(message)
        self.record = record


def coordinate_header(header: bytes) -> bytes:
    """the BAM header `header` (magic, l_text, text, n_ref, references) saying SO:coordinate: the SO value of its @HD line
    replaced, SO:coordinate appended to an @HD line without one, `@HD VN:1.6 SO:coordinate` put in front of a text without
    an @HD line; l_text adjusted, everything else byte for byte.  A header that says so already is returned as it is."""
    l_text = struct.unpack_from("<i", header, 4)[0]
    text, rest = header[8:8 + l_text], header[8 + l_text:]
    if text.startswith(b"@HD\t") or text.startswith(b"@HD\n") or text.rstrip(b"\0") == b"@HD":
        end = len(text.rstrip(b"\0"))
        nl = text.find(b"\n", 0, end)
        stop = end if nl < 0 else nl
        fields = text[:stop].split(b"\t")
        if b"SO:coordinate" in fields[1:]:
            return header
        if any(f.startswith(b"SO:") for f in fields[1:]):
            fields = fields[:1] + [b"SO:coordinate" if f.startswith(b"SO:") else f for f in fields[1:]]
        else:
            fields.append(b"SO:coordinate")
        text = b"\t".join(fields) + text[stop:]
    else:
        text = b"@HD\tVN:1.6\tSO:coordinate\n" + text
    return header[:4] + struct.pack("<i", len(text)) + text + rest


def record_of(read) -> bytes:
    """The record AlignmentFile.write puts behind the others for `read`, block_size first: the record as it was read, without its
    sequence and qualities (l_seq = 0; `bin` stays the original's), its tag area the original's without the names set_tag was
    given, those appended in the order they were set.  (The one assembly: the file writer and RecordSink both call it.)"""
    raw = read._raw
    l_read_name, n_cigar = raw[8], struct.unpack_from("<H", raw, 12)[0]
    body_end = 32 + l_read_name + 4 * n_cigar
    tags = read._tagbytes
    for key in read._set_tags or ():
        tags = _without_tag(tags, key)
    for key in read._set_tags or ():
        tags += _encode_tag(key, read._tags[key])
    rec = raw[:16] + b"\0\0\0\0" + raw[20:body_end] + tags
    return struct.pack("<i", len(rec)) + rec


def whole_record(record_bytes) -> bytes:
    """what write_raw takes: one whole record, block_size and block_size bytes"""
    if len(record_bytes) < 36 or struct.unpack_from("<i", record_bytes, 0)[0] != len(record_bytes) - 4:
        raise ValueError("write_raw takes one whole record: block_size and block_size bytes")
    return bytes(record_bytes)


class RecordSink:
    """A write-only stand-in for the `-w` writer that keeps what it is given: write(read), write_raw(bytes) and close() as
    AlignmentFile has them in mode 'wb', the records side by side in `data`, record i being data[offsets[i] : offsets[i + 1]] --
    byte for byte what the file writer would have handed to its BGZF layer (record_of, whole_record).  The sharded `-w` run
    (sharded.py) gives every rank one and gathers them."""

    def __init__(self):
        self.data = bytearray()
        self.offsets = [0]
        self.closed = False

    def write(self, read) -> None:
        self.write_raw(record_of(read))

    def write_raw(self, record_bytes) -> None:
        if self.closed:
            raise IOError("the record sink is closed")
        self.data += whole_record(record_bytes)
        self.offsets.append(len(self.data))

    def close(self) -> None:
        self.closed = True


class _RecordHold:
    """stands where an AlignmentFile's BgzfWriter stands while sort= / index= hold the records: write_record puts the record
    behind the header in ONE growing buffer (the stream close() works on: no second copy is made of it) and notes where it
    ends; close() hands buffer and offsets to `finish`, once"""

    def __init__(self, header: bytes, finish):
        self.data = bytearray(header)
        self.offsets = [len(header)]        # record i is data[offsets[i] : offsets[i + 1]]
        self._finish = finish

    def write_record(self, data: bytes) -> None:
        self.data += data
        self.offsets.append(len(self.data))

    def extend(self, data, rec_off, chosen) -> None:
        """the records `chosen` (rising indices) of data / rec_off (AlignmentFile.write_raw_many) behind the others: their bytes in
        one piece where they are all of them, else gathered run by run of neighbours (numpy: nothing per record)"""
        import numpy as np
        if len(chosen) == 0:
            return
        lens = (rec_off[1:] - rec_off[:-1])[chosen]
        if len(chosen) == rec_off.shape[0] - 1:
            piece = memoryview(data)[int(rec_off[0]):int(rec_off[-1])]
        else:
            src = np.frombuffer(data, np.uint8)
            # a run: chosen records that are neighbours in `data`; one slice each
            heads = np.flatnonzero(np.concatenate(([True], chosen[1:] != chosen[:-1] + 1)))
            tails = np.concatenate((heads[1:], [len(chosen)])) - 1
            lo, hi = rec_off[:-1][chosen[heads]].tolist(), rec_off[1:][chosen[tails]].tolist()
            piece = np.concatenate([src[a:b] for a, b in zip(lo, hi)]).tobytes() if len(lo) > 1 else bytes(src[lo[0]:hi[0]])
        base = self.offsets[-1]
        self.data += piece
        self.offsets.extend((base + np.cumsum(lens)).tolist())

    def close(self) -> None:
        finish, self._finish = self._finish, None
        if finish is not None:
            data, offsets = self.data, self.offsets
            self.data, self.offsets = bytearray(), [0]
            finish(data, offsets)


class AlignmentFile:
    """BAM file opened for reading, with its .bai or .csi index when present."""

    def __init__(self, path: str, mode: str = "rb", template=None, **kwargs):
        if "c" in mode or path.endswith(".cram"):
            raise NotImplementedError("this class reads BAM: a CRAM is opened with cram.CramFile (open_alignment_file does)")
        self.filename = path
        self._writer = None
        if mode.startswith("w"):
            if mode != "wb":
                raise NotImplementedError("only BAM output (mode 'wb') is written")
            self._open_for_writing(path, kwargs.get("template", template), kwargs.get("deflate", "zlib"), kwargs.get("device", 0),
                                   kwargs.get("huffman", "fixed"), kwargs.get("sort", False), kwargs.get("index", None),
                                   kwargs.get("index_path", None), kwargs.get("csi", False))
            return
        self._bgzf = BgzfReader(path, verify=bool(kwargs.get("verify", False)))
        raw = []        # the header as it lies in the file: a file opened 'wb' with this one as template starts with these bytes

        def read(n):
            data = self._bgzf.read(n)
            raw.append(data)
            return data
        if read(4) != b"BAM\1":
            raise IOError("%s is not a BAM file" % path)
        l_text = struct.unpack("<i", read(4))[0]
        self.text = read(l_text).split(b"\0", 1)[0].decode("ascii", "replace")
        n_ref = struct.unpack("<i", read(4))[0]
        refs, lens = [], []
        for _ in range(n_ref):
            l_name = struct.unpack("<i", read(4))[0]
            refs.append(read(l_name)[:-1].decode("ascii"))
            lens.append(struct.unpack("<i", read(4))[0])
        self._header_bytes = b"".join(raw)
        self.references = tuple(refs)
        self.lengths = tuple(lens)
        self._tid = {r: i for i, r in enumerate(refs)}
        self._first_record = self._bgzf.tell()
        self.header = self._parse_header(self.text)
        self._index = None
        self._index_stats = None
        self._index_scheme = None         # (kind "bai" | "csi", min_shift, depth)
        # .bai first: a call that found its index before .csi was read opens the same file as before (htslib would take a
        # .csi first; the answers are the same).  What a file is, its magic says, not its name.
        stem = os.path.splitext(path)[0]
        for cand in (path + ".bai", stem + ".bai", path + ".csi", stem + ".csi"):
            if os.path.exists(cand):
                self._load_index(cand)
                break

    @staticmethod
    def _parse_header(text: str) -> Dict[str, list]:
        hdr: Dict[str, list] = {}
        for line in text.splitlines():
            if not line.startswith("@") or line.startswith("@CO"):
                continue
            parts = line.split("\t")
            rec = {}
            for f in parts[1:]:
                if len(f) >= 3 and f[2] == ":":
                    rec[f[:2]] = f[3:]
            hdr.setdefault(parts[0][1:], []).append(rec)
        return hdr

    def _load_index(self, path: str):
        with open(path, "rb") as f:
            data = f.read()
        if data[:2] == b"\x1f\x8b":
            self._load_csi(path)
        else:
            self._load_bai(path, data)

    def _load_bai(self, path: str, data: bytes):
        if data[:4] != b"BAI\1":
            raise IOError("%s is not a BAI index" % path)
        off = 4
        n_ref = struct.unpack_from("<i", data, off)[0]; off += 4
        index = []
        mapped = unmapped = 0
        for _ in range(n_ref):
            n_bin = struct.unpack_from("<i", data, off)[0]; off += 4
            bins: Dict[int, List[Tuple[int, int]]] = {}
            for _ in range(n_bin):
                b, n_chunk = struct.unpack_from("<Ii", data, off); off += 8
                chunks = list(struct.iter_unpack("<QQ", data[off:off + 16 * n_chunk])); off += 16 * n_chunk
                if b == 37450:  # pseudo-bin: [unmapped beg/end], [n_mapped, n_unmapped]
                    if len(chunks) >= 2:
                        mapped += chunks[1][0]
                        unmapped += chunks[1][1]
                else:
                    bins[b] = chunks
            n_intv = struct.unpack_from("<i", data, off)[0]; off += 4
            linear = list(struct.unpack_from("<%dQ" % n_intv, data, off)); off += 8 * n_intv
            index.append((bins, linear, None))
        if off + 8 <= len(data):
            unmapped += struct.unpack_from("<Q", data, off)[0]
        self._index = index
        self._index_stats = (mapped, unmapped)
        self._index_scheme = ("bai", 14, 5)

    def _load_csi(self, path: str):
        """A CSI index (CSIv1): a BGZF file, read through BgzfReader with every member's CRC32 checked.  Per reference the bins
        with their chunks and one `loffset` each instead of a linear index; the pseudo-bin and n_no_coor as in a BAI."""
        try:
            z = BgzfReader(path, verify=True)
            try:
                parts = []
                while True:
                    part = z.read(1 << 20)
                    if not part:
                        break
                    parts.append(part)
            finally:
                z.close()
        except (IOError, zlib.error, struct.error) as e:
            raise IOError("%s: the BGZF layer of the index does not inflate (%s)" % (path, e))
        data = b"".join(parts)
        if data[:4] != b"CSI\1":
            raise IOError("%s is not a CSI index (wrong magic behind the BGZF layer)" % path)
        try:
            min_shift, depth, l_aux = struct.unpack_from("<iii", data, 4)
            if min_shift < 0 or depth < 0 or min_shift + 3 * depth > 62 or depth > 10:
                raise IOError("%s: CSI min_shift / depth out of range (%d, %d)" % (path, min_shift, depth))
            if l_aux < 0:
                raise IOError("%s: negative count in CSI (l_aux)" % path)
            off = 16 + l_aux
            n_ref = struct.unpack_from("<i", data, off)[0]; off += 4
            if n_ref < 0:
                raise IOError("%s: negative count in CSI (n_ref)" % path)
            pseudo = _pseudo_bin(depth)
            index = []
            mapped = unmapped = 0
            for _ in range(n_ref):
                n_bin = struct.unpack_from("<i", data, off)[0]; off += 4
                if n_bin < 0:
                    raise IOError("%s: negative count in CSI (n_bin)" % path)
                bins: Dict[int, List[Tuple[int, int]]] = {}
                loffset: Dict[int, int] = {}
                for _ in range(n_bin):
                    b, loff, n_chunk = struct.unpack_from("<IQi", data, off); off += 16
                    if n_chunk < 0:
                        raise IOError("%s: negative count in CSI (n_chunk)" % path)
                    if off + 16 * n_chunk > len(data):
                        raise IOError("%s: truncated CSI (chunks)" % path)
                    chunks = list(struct.iter_unpack("<QQ", data[off:off + 16 * n_chunk])); off += 16 * n_chunk
                    if b == pseudo:
                        if len(chunks) >= 2:
                            mapped += chunks[1][0]
                            unmapped += chunks[1][1]
                    else:
                        bins[b] = chunks
                        loffset[b] = loff
                index.append((bins, None, loffset))
            if off + 8 <= len(data):
                unmapped += struct.unpack_from("<Q", data, off)[0]
        except struct.error:
            raise IOError("%s: truncated CSI" % path)
        self._index = index
        self._index_stats = (mapped, unmapped)
        self._index_scheme = ("csi", min_shift, depth)

    def index_info(self) -> Optional[dict]:
        """which index was loaded: {"kind": "bai" | "csi", "min_shift", "depth"}, or None without one"""
        if self._index_scheme is None:
            return None
        kind, min_shift, depth = self._index_scheme
        return {"kind": kind, "min_shift": min_shift, "depth": depth}

    def _min_offset(self, tid: int, beg: int) -> int:
        """An offset no record overlapping [beg, ...) lies in front of.  BAI: the linear index's entry of beg's 16-kbp window.
        CSI: htslib's rule -- the loffset of the leaf bin holding beg, else of the nearest present bin met by stepping to the
        previous sibling and, from a first sibling, to the parent; 0 when none is present."""
        _bins, linear, loffset = self._index[tid]
        _kind, min_shift, depth = self._index_scheme
        if loffset is None:
            if not linear:
                return 0
            li = beg >> 14
            return linear[li] if li < len(linear) else linear[-1]
        if not loffset:
            return 0
        b = ((1 << (3 * depth)) - 1) // 7 + (min(beg, (1 << (min_shift + 3 * depth)) - 1) >> min_shift)
        while True:
            if b in loffset:
                return loffset[b]
            if b == 0:
                return 0
            parent = (b - 1) >> 3
            b = b - 1 if b > (parent << 3) + 1 else parent

    @property
    def mapped(self) -> int:
        if self._index_stats is None:
            raise ValueError("mapping information not recorded in index or index not available")
        return self._index_stats[0]

    @property
    def unmapped(self) -> int:
        if self._index_stats is None:
            raise ValueError("mapping information not recorded in index or index not available")
        return self._index_stats[1]

    def gettid(self, reference: str) -> int:
        return self._tid.get(reference, -1)

    def get_reference_name(self, tid: int) -> str:
        return self.references[tid]

    def close(self):
        if self._writer is not None:
            self._writer.close()
            return
        self._bgzf.close()

    # ---- writing (mode 'wb')
    _held = None            # (sort= / index=) the _RecordHold that stands where the BgzfWriter stands until close()
    _device_fold = True     # (deflate="device", csi) the CSI fold on the GPU; False: svt_csi_build_bam on the host (tools/csi_ab.py's other leg)

    def _open_for_writing(self, path: str, template, deflate: str = "zlib", device: int = 0, huffman: str = "fixed", sort: bool = False,
                          index=None, index_path=None, csi: bool = False):
        """pysam.AlignmentFile(path, 'wb', template): the template's header text and reference list, byte for byte.  `deflate`,
        `device`, `huffman`: who compresses the members, and into which block (BgzfWriter).

        `sort=True` (`--sort-alignment`) and `index="bai"` (`--bai`).  With either, nothing is written before close(): the writer
        keeps the header and every record, which costs host memory equal to the inflated size of the file, and close() works
        on them as one piece -- their span table (svtyper_amd/csrc/svt_bam_sort_rules.h: key = tid' << 33 | (pos + 1) << 1 |
        reverse, tid' = n_ref for a record without coordinate; the record's extent on the reference), with `sort` the records in
        stable order by key and SO:coordinate in the header's @HD line, the members cut exactly where they are cut for records
        written in that order, and with `index` the .bai at `index_path` (default: path + ".bai").  With deflate="device" the
        header and the records go to the GPU once and the table, the sort, the gather and the members are made there
        (svt_bam_sorted_bgzf_device); otherwise on the host, by the same source.  The .bai fold is host code either way
        (svt_bai_build).

        `csi=True` (`--alignment-csi`): the index asked for, in the CSI container (as pysam's tabix_index(..., csi=True) and
        `samtools index -c` spell it) -- a CSIv1 index in the scheme (14, depth) whose depth is the smallest >= 5 that covers
        the header's longest reference, BGZF-compressed, at `index_path` (default: path + ".csi").  It holds records beyond
        2^29.  With deflate="device" its fold runs on the GPU behind the members (svt_bam_sorted_bgzf_csi_device), otherwise on
        the host (svt_csi_build_bam): the same bytes.  `index="csi"` is not a spelling of it (ValueError), and `csi=True` without
        `index` is a ValueError.  An index of an earlier file is removed in either format, .bai and .csi.  A record that cannot be sorted or indexed makes close() raise BamOrderError; with `index` and
        without `sort`, records that are not in key order do so once the BAM is complete, and no index is left behind.
        Without either option the writer streams as it always did."""
        header = getattr(template, "_header_bytes", None)
        if header is None:
            raise TypeError("mode 'wb' needs template=: an AlignmentFile of this module opened for reading")
        if index not in (None, "bai"):
            raise ValueError("index must be None or 'bai', not %r" % (index,))
        if csi and index is None:
            raise ValueError("csi=True says which container the index goes into: it needs index='bai'")
        self.text, self.header = template.text, template.header
        self.references, self.lengths = template.references, template.lengths
        self._tid = dict(template._tid)
        self._writer = BgzfWriter(path, deflate=deflate, device=device, huffman=huffman)
        if sort or index is not None:
            self._sort, self._index, self._csi = bool(sort), index, bool(csi)
            self._index_path = (os.fspath(path) + (".csi" if csi else ".bai") if index_path is None else index_path) if index is not None else None
            self._stale = (os.fspath(path) + ".bai", os.fspath(path) + ".csi") if index is not None else ()
            self._header_out = coordinate_header(header) if sort else header
            self._bgzf_out = self._writer
            self._held = self._writer = _RecordHold(self._header_out, self._close_held)
            return
        self._writer.write(header)
        self._writer.flush()            # (records start in a block of their own, as htslib leaves them)

    def _close_held(self, data: bytearray, offsets: List[int]) -> None:
        """the header and the held records as one piece: span table, order, members, index -- what bgzf.close_held asks of
        its writer.  `data`: the header and the records behind it; record i is data[offsets[i] : offsets[i + 1]]"""
        import numpy as np

        from . import native_reads as nr
        header_len, n = offsets[0], len(offsets) - 1
        n_ref = struct.unpack_from("<i", data, 8 + struct.unpack_from("<i", data, 4)[0])[0]
        rec_off = np.array(offsets, np.uint64)

        l_ref_max = max(self.lengths, default=0)
        folded = []                         # (deflate="device", csi) what the device fold behind the members left: (bytes, bad, kind)

        def members(w):
            """-> (the spans as written, the order they were written in)"""
            if w._deflate == "device" and self._index and self._csi and self._device_fold:
                made, _off, _start, spans, perm, csi, ibad, ikind, bad, kind = nr.bam_sorted_bgzf_csi_device(data, rec_off, n_ref, l_ref_max, self._sort,
                                                                                                              w._huffman, w._device)
                if bad:
                    raise self._order_error(data, offsets, bad, kind)
                w._f.write(memoryview(made))
                folded.append((csi, ibad, ikind))
                return spans, perm
            if w._deflate == "device":
                made, _off, _start, spans, perm, bad, kind = nr.bam_sorted_bgzf_device(data, rec_off, n_ref, self._sort, w._huffman, w._device)
                if bad:
                    raise self._order_error(data, offsets, bad, kind)
                w._f.write(memoryview(made))            # (the members as they came back: not copied again)
                return spans, perm
            view = memoryview(data)
            spans, _and, _or = nr.bam_spans(data, rec_off, n_ref)
            perm = np.arange(n, dtype=np.uint64)
            if self._sort:
                perm, bad, kind = nr.bam_sort_order(spans)
                if bad:
                    raise self._order_error(data, offsets, bad, kind)
                spans = spans[perm]
                spans["off"] = np.cumsum(spans["len"]) - spans["len"] + np.uint64(header_len)
            w.write(bytes(view[:header_len]))
            w.flush()
            for i in perm.tolist():
                w.write_record(bytes(view[offsets[i]:offsets[i + 1]]))     # (a record at a time: the stream is not doubled)
            return spans, perm

        def fold(held, log):
            if folded:
                return folded[0]
            starts, member_off = np.array(log.starts, np.uint64), np.array(log.offsets, np.uint64)
            if self._csi:
                return nr.csi_build_bam(held[0], n_ref, l_ref_max, starts, member_off)
            return nr.bai_build(held[0], n_ref, starts, member_off)

        def write_index(path, index):
            if self._csi:                   # (a .csi is BGZF, as a .tbi is)
                out = BgzfWriter(path)
                out.write(index)
                out.close()
                return
            with open(path, "wb") as f:
                f.write(index)
        close_held(self._bgzf_out, self._index_path, members, self._index and fold,
                   lambda held, bad, kind: self._order_error(data, offsets, int(held[1][bad - 1]) + 1, kind), write_index,
                   stale=self._stale if self._index else ())

    def _order_error(self, data, offsets, bad: int, kind: int) -> "BamOrderError":
        """`bad`: the 1-based number of the record among those handed to write() / write_raw()"""
        from . import native_reads as nr
        raw = bytes(data[offsets[bad - 1]:offsets[bad]])
        where = "record %d" % bad
        if len(raw) >= 36:
            tid, pos = struct.unpack_from("<ii", raw, 4)
            name = raw[36:36 + max(raw[12] - 1, 0)].decode("ascii", "replace")
            where = "record %d (%s, %d:%d)" % (bad, name, tid, pos)
        if kind == nr.BAM_KIND_TID:
            why = "its reference id is none of the header's %d" % len(self.references)
        elif kind == nr.BAM_KIND_POS:
            why = "its position is negative"
        elif kind == nr.BAM_KIND_RECORD:
            why = "its fixed part, name and CIGAR do not fit inside its block_size"
        elif kind == nr.BAM_KIND_BEYOND and getattr(self, "_csi", False):
            depth = nr.csi_depth(max(self.lengths, default=0))
            return BamOrderError("%s: %s ends beyond 2^%d, the limit of the .csi index's scheme (min_shift 14, depth %d, from the header's "
                                 "longest reference): it lies beyond its header's contigs; no index was written"
                                 % (self.filename, where, 14 + 3 * depth, depth), bad)
        elif kind == nr.BAM_KIND_BEYOND:
            return BamOrderError("%s: %s ends beyond 2^29, which a .bai index cannot address (a CSI index is not written: ask for one "
                                 "with --alignment-csi (csi=True))" % (self.filename, where), bad)
        else:
            return BamOrderError("%s: %s is out of order (its key lies below the record in front): a %s index needs a "
                                 "coordinate-sorted BAM; no index was written -- use --sort-alignment (sort=True)"
                                 % (self.filename, where, ".csi" if getattr(self, "_csi", False) else ".bai"), bad)
        return BamOrderError("%s: %s cannot be sorted or indexed (%s)" % (self.filename, where, why), bad)

    def write(self, read: AlignedSegment) -> None:
        """One record behind the others: the record as it was read, without its sequence and qualities (l_seq = 0; `bin` stays
        the original's), its tag area the original's without the names set_tag was given, those appended in the order they
        were set.  A one-character string goes out as type A (XV:A:R, what `svtyper -w` sets), a longer one as Z, an int as i,
        a float as f."""
        if self._writer is None:
            raise IOError("%s is not open for writing" % self.filename)
        self._writer.write_record(record_of(read))

    def write_raw(self, record_bytes: bytes) -> None:
        """One FINISHED record behind the others -- its block_size and everything behind it, as write() would have put it
        together (the device reader's evidence dump hands over such records) -- through the same BgzfWriter.write_record."""
        if self._writer is None:
            raise IOError("%s is not open for writing" % self.filename)
        self._writer.write_record(whole_record(record_bytes))

    def write_raw_many(self, data, rec_off, keep=None) -> None:
        """FINISHED records side by side -- record i is data[rec_off[i] : rec_off[i + 1]] (n + 1 offsets, block_size first, as
        write_raw takes them one at a time) --, those with keep[i] != 0 (all of them without `keep`), in that order.  A writer that
        holds its records (sort= / index=) takes the kept bytes and their offsets in one append: no Python runs per record, and the
        records are checked where close() makes their span table.  A streaming writer hands them to write_raw one by one."""
        import numpy as np
        if self._writer is None:
            raise IOError("%s is not open for writing" % self.filename)
        rec_off = np.ascontiguousarray(rec_off, np.int64)
        n = rec_off.shape[0] - 1
        if n < 0 or rec_off[0] < 0 or rec_off[-1] > len(data) or (np.diff(rec_off) < 0).any():
            raise ValueError("write_raw_many: rec_off holds n + 1 rising offsets into data")
        if keep is not None and len(keep) != n:
            raise ValueError("write_raw_many: keep holds one entry per record")
        chosen = np.arange(n) if keep is None else np.flatnonzero(np.asarray(keep))
        if self._held is not None:
            if len(chosen):             # what write_raw asks of a record, of all of them at once
                lo, lens = rec_off[:-1][chosen], (rec_off[1:] - rec_off[:-1])[chosen]
                if (lens < 36).any():
                    raise ValueError("write_raw takes one whole record: block_size and block_size bytes")
                src = np.frombuffer(data, np.uint8)
                size = (src[lo].astype(np.int64) | src[lo + 1].astype(np.int64) << 8 | src[lo + 2].astype(np.int64) << 16
                        | src[lo + 3].astype(np.int64) << 24)
                if (size != lens - 4).any():
                    raise ValueError("write_raw takes one whole record: block_size and block_size bytes")
            self._held.extend(data, rec_off, chosen)
            return
        view = memoryview(data)
        lo, hi = rec_off[:-1][chosen].tolist(), rec_off[1:][chosen].tolist()
        for a, b in zip(lo, hi):
            self.write_raw(view[a:b])

    # ---- iteration
    def _next_record(self) -> Optional[AlignedSegment]:
        szb = self._bgzf.read(4)
        if len(szb) < 4:
            return None
        size = struct.unpack("<i", szb)[0]
        data = self._bgzf.read(size)
        if len(data) < size:
            return None
        return AlignedSegment(self, data)

    def fetch(self, contig: Optional[str] = None, start=None, stop=None, **kwargs) -> Iterator[AlignedSegment]:
        """Reads overlapping [start, stop) in coordinate order; all reads when contig is None."""
        reference = kwargs.get("reference", contig)
        if "end" in kwargs and stop is None:
            stop = kwargs["end"]
        if reference is None:
            self._bgzf.seek(self._first_record)
            while True:
                r = self._next_record()
                # pysam walks an indexed file reference by reference (IteratorRowAllRefs): the unplaced unmapped
                # reads at the end of a coordinate-sorted BAM (reference id -1) are never yielded
                if r is None or r.reference_id < 0:
                    return
                yield r
        tid = self.gettid(reference)
        if tid < 0:
            raise ValueError("invalid contig `%s`" % reference)
        beg = 0 if start is None else max(0, int(start))
        end = self.lengths[tid] if stop is None else int(stop)
        if end <= beg:
            return
        if self._index is None:
            raise ValueError("fetch called on bamfile without index")
        bins = self._index[tid][0]
        _kind, min_shift, depth = self._index_scheme
        # the window as the index sees it: clipped to the positions its scheme covers and to the contig
        bin_end = min(end, 1 << (min_shift + 3 * depth))
        if self.lengths[tid] > 0:
            bin_end = min(bin_end, self.lengths[tid])
        if bin_end <= beg:
            return
        min_off = self._min_offset(tid, beg)
        chunks = []
        for b in _reg2bins(beg, bin_end, min_shift, depth):
            for cb, ce in bins.get(b, ()):
                if ce > min_off:
                    chunks.append((cb, ce))
        if not chunks:
            return
        chunks.sort()
        merged = [list(chunks[0])]
        for cb, ce in chunks[1:]:
            if cb <= merged[-1][1]:
                if ce > merged[-1][1]:
                    merged[-1][1] = ce
            else:
                merged.append([cb, ce])
        for cb, ce in merged:
            self._bgzf.seek(cb)
            while self._bgzf.tell() < ce:
                r = self._next_record()
                if r is None:
                    break
                if r.reference_id != tid or r.reference_start >= end:
                    return
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


def open_alignment_file(path: str, reference_fasta: Optional[str] = None, verify: bool = False, cram_codec: str = "host", device: int = 0):
    """pysam.AlignmentFile when pysam is importable, else the built-in BAM reader or, for a *.cram, the built-in CRAM reader
    (svtyper/singlesample.py:53-62 semantics: the extension decides).  `verify`: the built-in reader, checking the CRC32 of
    every BGZF block it inflates, or of every CRAM container header and block it reads (the drivers' verify="crc32").
    `cram_codec`, `device`: who decodes a CRAM's rANS blocks (cram.CramFile)."""
    if not (path.endswith(".bam") or path.endswith(".cram")):
        raise ValueError("Error: %s is not a valid alignment file (*.bam or *.cram)" % path)
    if verify and path.endswith(".bam"):
        return AlignmentFile(path, "rb", verify=True)
    if path.endswith(".cram") and (verify or cram_codec != "host"):     # (what pysam has no word for: the built-in reader)
        from .cram import CramFile
        return CramFile(path, verify=verify, codec=cram_codec, device=device)
    try:
        import pysam  # type: ignore
        if path.endswith(".bam"):
            return pysam.AlignmentFile(path, mode="rb")
        return pysam.AlignmentFile(path, mode="rc", reference_filename=reference_fasta)
    except ImportError:
        if path.endswith(".cram"):
            from .cram import CramFile
            return CramFile(path, codec=cram_codec, device=device)
        return AlignmentFile(path, "rb")

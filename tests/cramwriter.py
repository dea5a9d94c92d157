"""A CRAM 3.0 WRITER for the tests, made from the format's published text (CRAM format specification 3.0) and sharing no code
with svtyper_amd/cram.py or the native decoders: its own ITF8 / LTF8, bit writer, canonical Huffman, rANS 4x8 encoder and .crai
writer.  `write_cram` turns BAM records into a CRAM file whose layout a `Layout` says: the encoding of every series, core or
external placement, shared blocks, the block method of every block, names kept or not, mates attached or detached, AP as delta
or absolute, records per slice, slices per container, multi-reference slices -- and damaged variants.

Bases and qualities are not in the records' meaning here: the writer stores `N` and 0xFF where a series wants them.
"""
from __future__ import annotations

import bz2
import gzip
import heapq
import lzma
import struct
import zlib
from collections import Counter
from typing import Dict, List, Optional, Tuple

RAW, GZIP, BZIP2, LZMA, RANS0, RANS1 = 0, 1, 2, 3, 4, 41     # block methods (RANS1: method 4, order 1)


# ------------------------------------------------------------------------------------------ numbers and bits
def itf8(v: int) -> bytes:
    v &= 0xFFFFFFFF
    if v < 0x80:
        return bytes([v])
    if v < 0x4000:
        return bytes([0x80 | v >> 8, v & 0xFF])
    if v < 0x200000:
        return bytes([0xC0 | v >> 16, v >> 8 & 0xFF, v & 0xFF])
    if v < 0x10000000:
        return bytes([0xE0 | v >> 24, v >> 16 & 0xFF, v >> 8 & 0xFF, v & 0xFF])
    return bytes([0xF0 | v >> 28, v >> 20 & 0xFF, v >> 12 & 0xFF, v >> 4 & 0xFF, v & 0x0F])


def ltf8(v: int) -> bytes:
    v &= 0xFFFFFFFFFFFFFFFF
    for extra in range(8):
        if v < 1 << (7 * (extra + 1)):
            head = (0xFF << (8 - extra)) & 0xFF | v >> (8 * extra)
            return bytes([head]) + bytes((v >> (8 * k)) & 0xFF for k in range(extra - 1, -1, -1))
    return b"\xff" + v.to_bytes(8, "big")


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value: int, bits: int) -> None:
        for k in range(bits - 1, -1, -1):
            self.acc = self.acc << 1 | (value >> k & 1)
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc = self.n = 0

    def done(self) -> bytes:
        if self.n:
            return bytes(self.out) + bytes([self.acc << (8 - self.n)])
        return bytes(self.out)


# ------------------------------------------------------------------------------------------ rANS 4x8
def _normalise(counts: Dict[int, int]) -> Dict[int, int]:
    total = sum(counts.values())
    f = {s: max(1, c * 4096 // total) for s, c in counts.items()}
    while sum(f.values()) > 4096:
        s = max(f, key=lambda k: f[k])
        f[s] -= 1
    top = max(f, key=lambda k: f[k])
    f[top] += 4096 - sum(f.values())
    return f


def _table(f: Dict[int, int]) -> bytes:
    """the symbols in rising order; a symbol that follows its predecessor directly is followed by the count of further direct
    successors, which then come without their symbol byte"""
    out, rle = bytearray(), 0
    for s in range(256):
        if s not in f:
            continue
        if rle:
            rle -= 1
        else:
            out.append(s)
            if s and s - 1 in f:
                run = 0
                while s + run + 1 in f:
                    run += 1
                out.append(run)
                rle = run
        out += bytes([f[s]]) if f[s] < 128 else bytes([0x80 | f[s] >> 8, f[s] & 0xFF])
    out.append(0)
    return bytes(out)


class _Enc:
    """the four states and the bytes they emit, which the block holds in reverse"""

    def __init__(self):
        self.r = [1 << 23] * 4
        self.rev = bytearray()

    def put(self, j: int, start: int, freq: int) -> None:
        x = self.r[j]
        x_max = ((1 << 23) >> 12 << 8) * freq
        while x >= x_max:
            self.rev.append(x & 0xFF)
            x >>= 8
        self.r[j] = (x // freq << 12) + x % freq + start

    def done(self) -> bytes:
        for j in (3, 2, 1, 0):
            self.rev += self.r[j].to_bytes(4, "big")
        return bytes(reversed(self.rev))


def _cumulative(f: Dict[int, int]) -> Dict[int, int]:
    c, acc = {}, 0
    for s in sorted(f):
        c[s] = acc
        acc += f[s]
    return c


def rans_encode(data: bytes, order: int, bad_sum: bool = False) -> bytes:
    """one rANS 4x8 block: order, compressed size, uncompressed size, frequency table, states, bytes"""
    n = len(data)
    if order == 1 and n < 4:
        order = 0
    if n == 0:
        return bytes([0]) + struct.pack("<II", 0, 0)
    e = _Enc()
    if order == 0:
        f = _normalise(Counter(data))
        c = _cumulative(f)
        for i in range(n - 1, (n & ~3) - 1, -1):               # the last 1 to 3 symbols: states 0 .. 2
            e.put(i & 3, c[data[i]], f[data[i]])
        for i in range((n & ~3) - 1, -1, -1):
            e.put(i & 3, c[data[i]], f[data[i]])
        written = dict(f)
        if bad_sum:
            s = min(written)
            written[s] += -5 if written[s] > 5 else 5
        payload = _table(written) + e.done()
    else:
        q = n >> 2
        ctx_counts: Dict[int, Counter] = {}
        for j in range(4):
            last = 0
            for i in range(j * q, (j + 1) * q if j < 3 else n):
                ctx_counts.setdefault(last, Counter())[data[i]] += 1
                last = data[i]
        f1 = {ctx: _normalise(cnt) for ctx, cnt in ctx_counts.items()}
        c1 = {ctx: _cumulative(f) for ctx, f in f1.items()}
        for i in range(n - 1, 4 * q - 1, -1):                  # the remainder belongs to the last quarter
            ctx = data[i - 1]
            e.put(3, c1[ctx][data[i]], f1[ctx][data[i]])
        for t in range(q - 1, -1, -1):
            for j in (3, 2, 1, 0):
                i = j * q + t
                ctx = data[i - 1] if t else 0
                e.put(j, c1[ctx][data[i]], f1[ctx][data[i]])
        table, rle = bytearray(), 0
        for ctx in range(256):
            if ctx not in f1:
                continue
            if rle:
                rle -= 1
            else:
                table.append(ctx)
                if ctx and ctx - 1 in f1:
                    run = 0
                    while ctx + run + 1 in f1:
                        run += 1
                    table.append(run)
                    rle = run
            written = dict(f1[ctx])
            if bad_sum and ctx == min(f1):
                s = min(written)
                written[s] += -5 if written[s] > 5 else 5
            table += _table(written)
        table.append(0)
        payload = bytes(table) + e.done()
    return bytes([order]) + struct.pack("<II", len(payload), n) + payload


# ------------------------------------------------------------------------------------------ encodings
def _enc(kind: int, params: bytes) -> bytes:
    return itf8(kind) + itf8(len(params)) + params


def _huffman_lengths(counts: Counter) -> Dict[int, int]:
    if len(counts) == 1:
        return {next(iter(counts)): 0}
    heap = [(c, i, (s,)) for i, (s, c) in enumerate(sorted(counts.items()))]
    heapq.heapify(heap)
    depth = {s: 0 for s in counts}
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


class IntCodec:
    """how the values of one series (ints, or single bytes) are written: spec = ("external", cid) | ("huffman",) | ("beta",) |
    ("gamma",) | ("subexp", k) | ("null",) | ("golomb",) (a damaged variant: never used for values)"""

    def __init__(self, spec, values: List[int], as_byte: bool):
        self.spec, self.as_byte = spec, as_byte
        kind = spec[0]
        if not values and kind != "golomb":
            kind = "null"
        self.kind = kind
        if kind == "huffman":
            lengths = _huffman_lengths(Counter(values))
            order = sorted(lengths, key=lambda s: (lengths[s], s))
            self.codes, code, last = {}, 0, lengths[order[0]]
            for s in order:
                code <<= lengths[s] - last
                last = lengths[s]
                self.codes[s] = (code, last)
                code += 1
            self.header = _enc(3, itf8(len(order)) + b"".join(itf8(s) for s in order) + itf8(len(order)) + b"".join(itf8(lengths[s]) for s in order))
        elif kind == "beta":
            self.offset = -min(values)
            self.bits = max(max(values) + self.offset, 1).bit_length()
            self.header = _enc(6, itf8(self.offset) + itf8(self.bits))
        elif kind == "gamma":
            self.offset = 1 - min(values)
            self.header = _enc(9, itf8(self.offset))
        elif kind == "subexp":
            self.offset, self.k = -min(values), spec[1]
            self.header = _enc(7, itf8(self.offset) + itf8(self.k))
        elif kind == "external":
            self.header = _enc(1, itf8(spec[1]))
        elif kind == "golomb":
            self.header = _enc(2, itf8(0) + itf8(2))
        else:
            self.header = _enc(0, b"")

    def put(self, v: int, core: BitWriter, ext: Dict[int, bytearray]) -> None:
        if self.kind == "external":
            ext.setdefault(self.spec[1], bytearray()).extend(bytes([v & 0xFF]) if self.as_byte else itf8(v))
        elif self.kind == "huffman":
            core.put(*self.codes[v])
        elif self.kind == "beta":
            core.put(v + self.offset, self.bits)
        elif self.kind == "gamma":
            x = v + self.offset
            core.put(0, x.bit_length() - 1)
            core.put(x, x.bit_length())
        elif self.kind == "subexp":
            x = v + self.offset
            if x < 1 << self.k:
                core.put(0, 1)
                core.put(x, self.k)
            else:
                b = x.bit_length() - 1
                ones = b - self.k + 1
                core.put((1 << ones) - 1, ones)
                core.put(0, 1)
                core.put(x & ((1 << b) - 1), b)
        else:
            raise AssertionError("a value for a series encoded as %s" % self.kind)


class ArrayCodec:
    """byte arrays: spec = ("len", int spec of the lengths, int spec of the bytes) | ("stop", stop byte, cid)"""

    def __init__(self, spec, arrays: List[bytes]):
        self.spec = spec
        if not arrays:
            self.header = _enc(0, b"")
        elif spec[0] == "len":
            self.lens = IntCodec(spec[1], [len(a) for a in arrays], False)
            self.vals = IntCodec(spec[2], [x for a in arrays for x in a] or [0], True)
            self.header = _enc(4, self.lens.header + self.vals.header)
        else:
            assert all(spec[1] not in a for a in arrays), "the stop byte occurs in a value"
            self.header = _enc(5, bytes([spec[1]]) + itf8(spec[2]))

    def put(self, a: bytes, core: BitWriter, ext: Dict[int, bytearray]) -> None:
        if self.spec[0] == "len":
            self.lens.put(len(a), core, ext)
            for x in a:
                self.vals.put(x, core, ext)
        else:
            ext.setdefault(self.spec[2], bytearray()).extend(a + bytes([self.spec[1]]))


INT_SERIES = ("BF", "CF", "RI", "RL", "AP", "RG", "MF", "NS", "NP", "TS", "NF", "TL", "FN", "FP", "DL", "RS", "PD", "HC", "MQ")
BYTE_SERIES = ("FC", "BS", "BA", "QS")
ARRAY_SERIES = ("RN", "IN", "SC", "BB", "QQ")
_CID = {name: k + 1 for k, name in enumerate(INT_SERIES + BYTE_SERIES + ARRAY_SERIES)}
TAG_LEN_CID, TAG_VAL_CID = 60, 61


class Layout:
    """the knobs.  `ints` / `bytes_` / `arrays`: the spec of every series that is not named in `series` (a callable from the
    series' name to its spec, so that each can have a block of its own); `series`: specs by name; `tags`: the spec of the tag
    values, a callable from the tag's three characters; `methods`: block method by content id, `method` for the others, `core_method` for the
    core block."""

    def __init__(self, **kw):
        self.names = True
        self.attached = True
        self.ap_delta = True
        self.records_per_slice = 1000
        self.slices_per_container = 1
        self.multi_ref = False
        self.embedded_ref_flag = False
        self.feature_mix = False            # X, B, b, i, q and Q features inside M runs and for one-base insertions
        self.qual_array = False             # CF bit 1: QS x RL behind every record
        self.no_seq_unmapped = False        # CF bit 8 on unmapped records: no BA x RL
        self.ints = lambda name: ("external", _CID[name])
        self.bytes_ = lambda name: ("external", _CID[name])
        self.arrays = lambda name: ("len", ("external", _CID[name] + 30), ("external", _CID[name]))
        self.series: Dict[str, tuple] = {}
        self.tags = lambda tag: ("len", ("external", TAG_LEN_CID), ("external", TAG_VAL_CID))
        self.methods: Dict[int, int] = {}
        self.method = RAW
        self.core_method = RAW
        self.header_method = RAW
        self.damage: Optional[str] = None   # "crc" | "truncated" | "freq" | "method5" | "major2" | "golomb" | "past_block"
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError("no knob %s" % k)
            setattr(self, k, v)


def default_layout(**kw) -> Layout:
    """like what samtools writes by default: every series in an external block of its own, rANS order 0 for the numbers, order 1
    for names, qualities and tag values; 1 000 records per slice here"""
    methods = {cid: RANS0 for cid in range(1, 100)}
    for name in ("RN", "QS", "BA", "SC", "IN"):
        methods[_CID[name]] = RANS1
    methods[TAG_VAL_CID] = RANS1
    base = dict(methods=methods, method=RANS0, core_method=RAW, records_per_slice=1000, header_method=GZIP)
    base.update(kw)
    return Layout(**base)


# ------------------------------------------------------------------------------------------ records
class Rec:
    __slots__ = ("ref", "pos", "mapq", "flag", "l_seq", "next_ref", "next_pos", "tlen", "name", "cigar", "tags", "end")

    def __init__(self, raw: bytes):
        (self.ref, self.pos, l_name, self.mapq, _bin, n_cigar, self.flag, self.l_seq, self.next_ref, self.next_pos, self.tlen) = \
            struct.unpack_from("<iiBBHHHiiii", raw, 0)
        self.name = raw[32:32 + l_name - 1]
        at = 32 + l_name
        self.cigar = [(c & 0xF, c >> 4) for c in struct.unpack_from("<%dI" % n_cigar, raw, at)]
        at += 4 * n_cigar + (self.l_seq + 1) // 2 + self.l_seq
        self.tags = split_tags(raw[at:])
        span = sum(n for op, n in self.cigar if op in (0, 2, 3, 7, 8))
        self.end = self.pos + (span if span and not self.flag & 4 else 1)


_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def split_tags(b: bytes) -> List[Tuple[bytes, bytes]]:
    """[(the tag's two characters and its type, its value bytes as BAM holds them)]"""
    out, i = [], 0
    while i + 3 <= len(b):
        t = chr(b[i + 2])
        j = i + 3
        if t in _FIXED:
            j += _FIXED[t]
        elif t in "ZH":
            j = b.index(b"\0", j) + 1
        else:
            j += 5 + struct.unpack_from("<I", b, j + 1)[0] * _FIXED[chr(b[j])]
        out.append((b[i:i + 3], b[i + 3:j]))
        i = j
    return out


def chain_tlen(chain: List[Rec]) -> Optional[List[int]]:
    """the template lengths the format's text gives the records of an attached chain: rightmost end minus leftmost start plus 1
    (1-based, inclusive), positive for the record that starts leftmost (the earliest at equal starts), negative for the
    others; zeros when they are not all mapped to one reference"""
    if any(r.flag & 4 or r.ref < 0 or r.ref != chain[0].ref for r in chain):
        return [0] * len(chain)
    lo = min(r.pos for r in chain)
    hi = max(r.end for r in chain)
    first = next(k for k, r in enumerate(chain) if r.pos == lo)
    return [hi - lo if k == first else -(hi - lo) for k in range(len(chain))]


def _attachable(chain: List[Rec]) -> bool:
    want = chain_tlen(chain)
    for k, r in enumerate(chain):
        mate = chain[(k + 1) % len(chain)]
        if (r.next_ref, r.next_pos) != (mate.ref, mate.pos) or bool(r.flag & 0x20) != bool(mate.flag & 0x10) or bool(r.flag & 0x8) != bool(mate.flag & 0x4):
            return False
        if r.tlen != want[k]:
            return False
    return True


class _Slice:
    def __init__(self):
        self.events: List[Tuple[str, str, object]] = []      # (series or tag key, "int" | "byte" | "array", value)
        self.n = 0
        self.refs: List[Tuple[int, int, int]] = []           # per record (ref, pos, end)
        self.ref = -1
        self.counter = 0


def _features(r: Rec, mix: bool) -> List[tuple]:
    """(code, read position, payload) from the CIGAR; with `mix` also base-level features inside M runs, which add nothing"""
    out, rp = [], 1
    for op, n in r.cigar:
        if op in (0, 7, 8):
            if mix and n >= 6:
                out += [("Q", rp, 30), ("X", rp, 1), ("B", rp + 1, None), ("b", rp + 2, b"NN"), ("q", rp + 4, b"\x1e\x1e")]
            rp += n
        elif op == 1:
            out.append(("i", rp, None) if mix and n == 1 else ("I", rp, b"N" * n))
            rp += n
        elif op == 4:
            out.append(("S", rp, b"N" * n))
            rp += n
        else:
            out.append(({2: "D", 3: "N", 5: "H", 6: "P"}[op], rp, n))
    return out


def _slice_events(recs: List[Rec], counter: int, L: Layout, rg_index: Dict[bytes, int], tag_lists: Dict[tuple, int], multi: bool,
                  names_out: List[bytes]) -> _Slice:
    s = _Slice()
    s.n, s.counter = len(recs), counter
    s.ref = -2 if multi else recs[0].ref
    ev = s.events
    # chains: records of one name, in order, where the format can rebuild their mate fields
    link: Dict[int, int] = {}
    head: Dict[int, int] = {}
    if L.attached:
        by_name: Dict[bytes, List[int]] = {}
        for k, r in enumerate(recs):
            if r.flag & 1:
                by_name.setdefault(r.name, []).append(k)
        for ks in by_name.values():
            if len(ks) >= 2 and _attachable([recs[k] for k in ks]):
                for a, b in zip(ks[:-1], ks[1:]):
                    link[a] = b
                for k in ks:
                    head[k] = ks[0]
    start = 0 if multi else min((r.pos + 1 for r in recs), default=0)
    last = start
    for k, r in enumerate(recs):
        s.refs.append((r.ref, r.pos, r.end))
        attached = k in head
        plain = not attached and (r.next_ref, r.next_pos, r.tlen) == (-1, -1, 0) and not r.flag & 0x28
        # a record without its sequence (SEQ `*`) keeps the read length its CIGAR gives, under CF bit 8
        no_seq = r.l_seq == 0 and bool(r.cigar)
        rl = sum(n for op, n in r.cigar if op in (0, 1, 4, 7, 8)) if no_seq else r.l_seq
        cf = ((1 if L.qual_array and not no_seq else 0) | (0 if attached or plain else 2) | (4 if k in link else 0)
              | (8 if no_seq or (r.flag & 4 and L.no_seq_unmapped) else 0))
        ev.append(("BF", "int", r.flag & ~0x28 if attached else r.flag))
        ev.append(("CF", "int", cf))
        if multi:
            ev.append(("RI", "int", r.ref))
        ev.append(("RL", "int", rl))
        ev.append(("AP", "int", r.pos + 1 - last if L.ap_delta else r.pos + 1))
        if L.ap_delta:
            last = r.pos + 1
        tags = list(r.tags)
        rg = -1
        for t in tags:
            if t[0] == b"RGZ" and t[1][:-1] in rg_index:
                rg = rg_index[t[1][:-1]]
                tags.remove(t)
                break
        ev.append(("RG", "int", rg))
        if L.names:
            ev.append(("RN", "array", r.name))
            names_out.append(r.name)
        if cf & 2:
            ev.append(("MF", "int", (1 if r.flag & 0x20 else 0) | (2 if r.flag & 0x8 else 0)))
            if not L.names:
                ev.append(("RN", "array", r.name))
                names_out.append(r.name)
            ev += [("NS", "int", r.next_ref), ("NP", "int", r.next_pos + 1), ("TS", "int", r.tlen)]
        elif not L.names:
            names_out.append(str(counter + (head[k] if attached else k)).encode())
        if k in link:
            ev.append(("NF", "int", link[k] - k - 1))
        key = tuple(t[0] for t in tags)
        ev.append(("TL", "int", tag_lists.setdefault(key, len(tag_lists))))
        for t in tags:
            ev.append((t[0].decode("latin-1"), "array", t[1]))
        if not r.flag & 4:
            feats = _features(r, L.feature_mix)
            ev.append(("FN", "int", len(feats)))
            prev = 0
            for code, rp, payload in feats:
                ev.append(("FC", "byte", ord(code)))
                ev.append(("FP", "int", rp - prev))
                prev = rp
                if code == "B":
                    ev += [("BA", "byte", ord("N")), ("QS", "byte", 30)]
                elif code == "X":
                    ev.append(("BS", "byte", payload))
                elif code == "i":
                    ev.append(("BA", "byte", ord("N")))
                elif code == "Q":
                    ev.append(("QS", "byte", payload))
                elif code in "IbSq":
                    ev.append(({"I": "IN", "b": "BB", "S": "SC", "q": "QQ"}[code], "array", payload))
                else:
                    ev.append(({"D": "DL", "N": "RS", "H": "HC", "P": "PD"}[code], "int", payload))
            ev.append(("MQ", "int", r.mapq))
        elif not cf & 8:
            ev += [("BA", "byte", ord("N"))] * r.l_seq
        if cf & 1:
            ev += [("QS", "byte", 0xFF)] * r.l_seq
    return s


# ------------------------------------------------------------------------------------------ blocks and containers
def _compress(data: bytes, method: int, bad_sum: bool = False) -> Tuple[int, bytes]:
    if method == GZIP:
        return 1, gzip.compress(data)
    if method == BZIP2:
        return 2, bz2.compress(data)
    if method == LZMA:
        return 3, lzma.compress(data)
    if method in (RANS0, RANS1):
        return 4, rans_encode(data, 1 if method == RANS1 else 0, bad_sum)
    return 0, data


def block(method: int, ctype: int, cid: int, data: bytes, bad_sum: bool = False, wrong_crc: bool = False, as_method: Optional[int] = None) -> bytes:
    m, comp = _compress(data, method, bad_sum)
    body = bytes([m if as_method is None else as_method, ctype]) + itf8(cid) + itf8(len(comp)) + itf8(len(data)) + comp
    crc = zlib.crc32(body) & 0xFFFFFFFF
    return body + struct.pack("<I", crc ^ (0x5A5A if wrong_crc else 0))


def container(ref: int, start: int, span: int, n_records: int, counter: int, blocks: List[bytes], landmarks: List[int]) -> bytes:
    body = b"".join(blocks)
    head = (struct.pack("<i", len(body)) + itf8(ref) + itf8(start) + itf8(span) + itf8(n_records) + ltf8(counter) + ltf8(0) + itf8(len(blocks))
            + itf8(len(landmarks)) + b"".join(itf8(x) for x in landmarks))
    return head + struct.pack("<I", zlib.crc32(head) & 0xFFFFFFFF) + body


def eof_container() -> bytes:
    empty = itf8(1) + itf8(0)
    return container(-1, 4542278, 0, 0, 0, [block(RAW, 1, 0, empty * 3)], [])


def write_cram(path: str, header_text: str, records: List[bytes], layout: Optional[Layout] = None, crai: bool = True) -> dict:
    """`records`: BAM records without their block_size, in file order.  -> {"names": the name every record is to be read back
    with, "slices": [(container offset, landmark, records)], "containers": their offsets}"""
    L = layout or default_layout()
    recs = [Rec(r) for r in records]
    rg_index: Dict[bytes, int] = {}
    for line in header_text.splitlines():
        if line.startswith("@RG"):
            for f in line.split("\t")[1:]:
                if f.startswith("ID:"):
                    rg_index[f[3:].encode()] = len(rg_index)
    out = bytearray(b"CRAM" + bytes([2 if L.damage == "major2" else 3, 0]) + b"svtyper_amd test".ljust(20, b"\0"))
    text = header_text.encode("ascii")
    out += container(0, 0, 0, 0, 0, [block(L.header_method, 0, 0, struct.pack("<i", len(text)) + text)], [0])
    # slices: cut at reference changes unless multi-reference slices are asked for
    groups: List[List[Rec]] = []
    for r in recs:
        if groups and len(groups[-1]) < L.records_per_slice and (L.multi_ref or groups[-1][0].ref == r.ref):
            groups[-1].append(r)
        else:
            groups.append([r])
    names: List[bytes] = []
    info = {"names": names, "slices": [], "containers": []}
    index_lines: List[str] = []
    counter = 0
    k = 0
    first_data_block = True
    while k < len(groups):
        chunk = [groups[k]]
        while (len(chunk) < L.slices_per_container and k + len(chunk) < len(groups)
               and (L.multi_ref or groups[k + len(chunk)][0].ref == groups[k][0].ref)):
            chunk.append(groups[k + len(chunk)])
        k += len(chunk)
        tag_lists: Dict[tuple, int] = {}
        slices = []
        for g in chunk:
            slices.append(_slice_events(g, counter, L, rg_index, tag_lists, L.multi_ref, names))
            counter += len(g)
        # the codecs of the container: one per series, from the values of all its slices
        values: Dict[str, list] = {}
        kinds: Dict[str, str] = {}
        for s in slices:
            for key, kind, v in s.events:
                values.setdefault(key, []).append(v)
                kinds[key] = kind
        codecs: Dict[str, object] = {}
        for name in INT_SERIES + BYTE_SERIES:
            spec = L.series.get(name) or (L.ints(name) if name in INT_SERIES else L.bytes_(name))
            codecs[name] = IntCodec(spec, values.get(name, []), name in BYTE_SERIES)
        for name in ARRAY_SERIES:
            codecs[name] = ArrayCodec(L.series.get(name) or L.arrays(name), values.get(name, []))
        tag_keys = sorted(key for key in values if len(key) == 3)
        for key in tag_keys:
            codecs[key] = ArrayCodec(L.series.get(key) or L.tags(key), values[key])
        if L.damage == "golomb":
            codecs["MQ"].header = IntCodec(("golomb",), [], False).header      # (the values stay as they were: the reader stops at the header)
        td = b"".join(b"".join(key) + b"\0" for key in sorted(tag_lists, key=lambda t: tag_lists[t])) or b"\0"
        pres = [b"RN" + bytes([1 if L.names else 0]), b"AP" + bytes([1 if L.ap_delta else 0]), b"RR" + bytes([0 if L.embedded_ref_flag else 1]),
                b"SM" + bytes(5), b"TD" + itf8(len(td)) + td]
        pres_b = itf8(len(pres)) + b"".join(pres)
        series = [name.encode() + codecs[name].header for name in INT_SERIES + BYTE_SERIES + ARRAY_SERIES]
        series_b = itf8(len(series)) + b"".join(series)
        tags = [itf8(ord(key[0]) << 16 | ord(key[1]) << 8 | ord(key[2])) + codecs[key].header for key in tag_keys]
        tags_b = itf8(len(tags)) + b"".join(tags)
        comp = itf8(len(pres_b)) + pres_b + itf8(len(series_b)) + series_b + itf8(len(tags_b)) + tags_b
        blocks = [block(RAW, 1, 0, comp)]
        landmarks, at = [], len(blocks[0])
        slice_sizes = []
        for s in slices:
            core, ext = BitWriter(), {}
            for key, kind, v in s.events:
                codecs[key].put(v, core, ext)
            core_b = core.done()
            if L.damage == "past_block" and first_data_block:
                cid = max(ext, key=lambda c: len(ext[c]))
                ext[cid] = ext[cid][:len(ext[cid]) // 2]
            data_blocks = [block(L.core_method, 5, 0, core_b)]
            for cid in sorted(ext):
                method = L.methods.get(cid, L.method)
                first_rans = first_data_block and method in (RANS0, RANS1) and len(ext[cid]) > 0
                data_blocks.append(block(method, 4, cid, bytes(ext[cid]), bad_sum=L.damage == "freq" and first_rans,
                                         wrong_crc=L.damage == "crc" and first_data_block,
                                         as_method=5 if L.damage == "method5" and first_data_block else None))
                if first_rans or L.damage in ("crc", "method5"):
                    first_data_block = False
            if L.damage == "past_block":
                first_data_block = False
            placed = [x for x in s.refs if x[0] >= 0]
            lo = min((x[1] for x in placed), default=-1)
            hi = max((x[2] for x in placed), default=-1)
            one_ref = s.ref >= 0
            header = (itf8(s.ref) + itf8(lo + 1 if one_ref else 0) + itf8(hi - lo if one_ref else 0) + itf8(s.n) + ltf8(s.counter) + itf8(len(data_blocks))
                      + itf8(len(data_blocks)) + b"".join(itf8(0 if i == 0 else sorted(ext)[i - 1]) for i in range(len(data_blocks)))
                      + itf8(-1) + bytes(16))
            sl = [block(RAW, 2, 0, header)] + data_blocks
            landmarks.append(at)
            size = sum(len(b) for b in sl)
            slice_sizes.append(size)
            at += size
            blocks += sl
        all_refs = [x for s in slices for x in s.refs if x[0] >= 0]
        cref = -2 if L.multi_ref else slices[0].ref
        clo = min((x[1] for x in all_refs), default=-1) if cref >= 0 else -1
        chi = max((x[2] for x in all_refs), default=-1) if cref >= 0 else -1
        coff = len(out)
        info["containers"].append(coff)
        out += container(cref, clo + 1, chi - clo if cref >= 0 else 0, sum(s.n for s in slices), slices[0].counter, blocks, landmarks)
        for s, lm, size in zip(slices, landmarks, slice_sizes):
            info["slices"].append((coff, lm, s.n))
            seen: Dict[int, List[int]] = {}
            for ref, pos, end in s.refs:
                e = seen.setdefault(ref, [pos, end])
                e[0], e[1] = min(e[0], pos), max(e[1], end)
            for ref in seen:                # (file order: a sorted file's references rise; the unplaced come last)
                lo, hi = seen[ref]
                index_lines.append("%d\t%d\t%d\t%d\t%d\t%d" % (ref, lo + 1 if ref >= 0 else 0, hi - lo if ref >= 0 else 0, coff, lm, size))
    out += eof_container()
    if L.damage == "truncated":
        del out[info["containers"][-1] + 40:]
    with open(path, "wb") as f:
        f.write(bytes(out))
    if crai:
        with gzip.open(path + ".crai", "wb") as f:
            f.write(("\n".join(index_lines) + "\n").encode())
    return info

"""A token-level DEFLATE writer and a plain reference inflater (RFC 1951), for the inflate tests: pure Python, test code only.

Writer.  write(blocks) -> the raw-deflate payload of a list of blocks made by stored() / fixed() / dynamic() / bits().  A token is
  k                      a literal byte,
  (length, distance)     a match, (length, distance, length_symbol) to choose between symbol 284 + 30 and symbol 285 for 258,
  ("litsym", s)          the literal/length code of symbol s and nothing else (symbols no compressor writes: 286, 287, ...),
  ("distsym", s)         the distance code of symbol s and nothing else,
  ("bits", value, n)     n raw bits, lowest first.
dynamic() takes the code lengths as given (any set the caller wants, complete or not) or makes a complete, nearly flat set over
the symbols the tokens use; `header` forces HLIT / HDIST / HCLEN and how the code lengths are run-length coded ("none": no 16 / 17 /
18; "split": literal/length and distance lengths separately, as zlib's deflate does; "greedy": over both at once, so a repeat
may run from the literal lengths into the distance lengths; or `ops`, the list of (symbol, extra) itself).  BFINAL is set on the
last block.  expand(blocks) is what the tokens say the bytes are.

Reference.  inflate(payload, limit) reads the payload bit by bit with the RFC's own tables (a code is looked up by its length and
value, one bit at a time: no tables of prefixes, no bit buffer) and returns (ok, bytes, Profile).  The rules for a set of code
lengths are zlib's (inflate_table): over-subscribed never, incomplete only as one single code of one bit and not for the
code-length code, no codes at all only for distances.  `ok` is: the final block ended, nothing was wrong before it, and no more
than `limit` bytes came out.  The profile holds, per block, its type, symbol count (the end-of-block code not counted), stored
length and how often each code length was decoded; per match (out_pos, len, dist, lit_code_len, dist_code_len) and its total
bits, block and index in the block."""
import collections

LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
EOB = 256


class BitWriter:
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

    def align(self):
        self.n = (self.n + 7) // 8 * 8
        return self

    def raw(self, data):
        assert self.n % 8 == 0
        self.acc |= int.from_bytes(data, "little") << self.n
        self.n += 8 * len(data)
        return self

    def done(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def stored(data, nlen=None):
    return {"type": "stored", "data": bytes(data), "nlen": nlen}


def fixed(tokens, eob=True):
    return {"type": "fixed", "tokens": list(tokens), "eob": eob}


def dynamic(tokens, lit_lengths=None, dist_lengths=None, header=None, eob=True):
    return {"type": "dynamic", "tokens": list(tokens), "lit": lit_lengths, "dist": dist_lengths, "header": dict(header or {}), "eob": eob}


def bits(fields):
    """a 'block' of raw (value, count) fields, lowest bit first, with no header of its own"""
    return {"type": "bits", "fields": list(fields)}


def length_symbol(length):
    if length == 258:
        return 285
    s = max(k for k in range(28) if LENGTH_BASE[k] <= length)
    return 257 + s


def distance_symbol(dist):
    return max(k for k in range(30) if DIST_BASE[k] <= dist)


def canonical_codes(lengths):
    """{symbol: code} as RFC 1951 3.2.2 assigns them (the value is read first bit first)"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


def flat_lengths(used, size):
    """a complete set over the symbols `used`: with n of them and k = ceil(log2 n), 2^k - n codes of k - 1 bits, the rest k"""
    used = sorted(set(used))
    if len(used) == 1:                         # (one code alone would be an incomplete set: a second symbol nobody uses)
        used = sorted(set(used) | {0 if used[0] else 1})
    n = len(used)
    k = (n - 1).bit_length()
    short = (1 << k) - n
    lengths = [0] * size
    for i, s in enumerate(used):
        lengths[s] = k - 1 if i < short else k
    return lengths


def token_symbols(tokens):
    lit, dist = set(), set()
    for t in tokens:
        if isinstance(t, int):
            lit.add(t)
        elif t[0] == "litsym":
            lit.add(t[1])
        elif t[0] == "distsym":
            dist.add(t[1])
        elif t[0] != "bits":
            lit.add(t[2] if len(t) > 2 else length_symbol(t[0]))
            dist.add(distance_symbol(t[1]))
    return lit, dist


def run_length_ops(lengths, repeats=True):
    """code lengths -> [(symbol 0..18, extra)] as a greedy run-length coder writes them"""
    ops, i, n = [], 0, len(lengths)
    while i < n:
        v, run = lengths[i], 1
        while i + run < n and lengths[i + run] == v:
            run += 1
        if not repeats:
            ops += [(v, 0)] * run
        elif v == 0:
            left = run
            while left >= 11:
                take = min(left, 138)
                ops.append((18, take - 11))
                left -= take
            if left >= 3:
                ops.append((17, left - 3))
                left = 0
            ops += [(0, 0)] * left
        else:
            ops.append((v, 0))
            left = run - 1
            while left >= 3:
                take = min(left, 6)
                ops.append((16, take - 3))
                left -= take
            ops += [(v, 0)] * left
        i += run
    return ops


def expand_ops(ops):
    out = []
    for sym, extra in ops:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if sym == 17 else 11) + extra)
    return out


def op_spans(ops):
    """[(first, last + 1)] of the code lengths each op writes"""
    spans, at = [], 0
    for sym, extra in ops:
        n = 1 if sym < 16 else 3 + extra if sym < 18 else 11 + extra
        spans.append((at, at + n))
        at += n
    return spans


def dynamic_header(block):
    """(lit_lengths, dist_lengths, ops, cl_lengths, hclen) of a dynamic block: what its header is going to say"""
    h = block["header"]
    used_lit, used_dist = token_symbols(block["tokens"])
    lit = list(block["lit"]) if block["lit"] is not None else flat_lengths(used_lit | {EOB}, 286)
    dist = list(block["dist"]) if block["dist"] is not None else (flat_lengths(used_dist, 30) if len(used_dist) > 1 else
                                                                  [0] * min(used_dist) + [1] if used_dist else [0])
    hlit = h.get("hlit", max(257, max((s + 1 for s, l in enumerate(lit) if l), default=257)))
    hdist = h.get("hdist", max(1, max((s + 1 for s, l in enumerate(dist) if l), default=1)))
    lit = (lit + [0] * 286)[:hlit] if len(lit) <= hlit else lit[:hlit]
    dist = (dist + [0] * 30)[:hdist] if len(dist) <= hdist else dist[:hdist]
    if "ops" in h:
        ops = list(h["ops"])
        assert expand_ops(ops) == lit + dist, "the forced ops do not spell the code lengths"
    else:
        mode = h.get("repeats", "split")
        ops = (run_length_ops(lit + dist, mode != "none") if mode in ("none", "greedy") else run_length_ops(lit) + run_length_ops(dist))
    cl = h.get("cl_lengths") or flat_lengths({s for s, _e in ops}, 19)
    need = max(k + 1 for k, s in enumerate(CL_ORDER) if cl[s])
    hclen = h.get("hclen", max(4, need))
    assert hclen >= need and 4 <= hclen <= 19
    return lit, dist, ops, cl, hclen


def _tokens(w, tokens, lit_lengths, dist_lengths, eob):
    lit_code, dist_code = canonical_codes(lit_lengths), canonical_codes(dist_lengths)
    for t in tokens:
        if isinstance(t, int):
            w.code(lit_code[t], lit_lengths[t])
        elif t[0] == "litsym":
            w.code(lit_code[t[1]], lit_lengths[t[1]])
        elif t[0] == "distsym":
            w.code(dist_code[t[1]], dist_lengths[t[1]])
        elif t[0] == "bits":
            w.bits(t[1], t[2])
        else:
            length, dist = t[0], t[1]
            s = t[2] if len(t) > 2 else length_symbol(length)
            extra = length - LENGTH_BASE[s - 257]
            assert 3 <= length <= 258 and 0 <= extra < 1 << LENGTH_EXTRA[s - 257]       # (284 + 31 is 258 too: zlib takes it)
            w.code(lit_code[s], lit_lengths[s])
            w.bits(extra, LENGTH_EXTRA[s - 257])
            d = distance_symbol(dist)
            assert 1 <= dist <= 32768
            w.code(dist_code[d], dist_lengths[d])
            w.bits(dist - DIST_BASE[d], DIST_EXTRA[d])
    if eob:
        w.code(lit_code[EOB], lit_lengths[EOB])


def write_bits(blocks, final=True):
    """(payload, bits used) of the blocks; BFINAL on the last one if `final`"""
    w = BitWriter()
    for k, b in enumerate(blocks):
        last = 1 if final and k == len(blocks) - 1 else 0
        if b["type"] == "bits":
            for value, count in b["fields"]:
                w.bits(value, count)
        elif b["type"] == "stored":
            n = len(b["data"])
            assert n <= 65535
            w.bits(last, 1).bits(0, 2).align().bits(n, 16).bits(n ^ 0xFFFF if b["nlen"] is None else b["nlen"], 16).raw(b["data"])
        elif b["type"] == "fixed":
            w.bits(last, 1).bits(1, 2)
            _tokens(w, b["tokens"], FIXED_LIT, FIXED_DIST, b["eob"])
        else:
            lit, dist, ops, cl, hclen = dynamic_header(b)
            w.bits(last, 1).bits(2, 2).bits(len(lit) - 257, 5).bits(len(dist) - 1, 5).bits(hclen - 4, 4)
            for s in CL_ORDER[:hclen]:
                w.bits(cl[s], 3)
            cl_code = canonical_codes(cl)
            for sym, extra in ops:
                w.code(cl_code[sym], cl[sym])
                if sym >= 16:
                    w.bits(extra, (2, 3, 7)[sym - 16])
            _tokens(w, b["tokens"], lit + [0] * (288 - len(lit)), dist + [0] * (32 - len(dist)), b["eob"])
    return w.done(), w.n


def write(blocks, final=True):
    return write_bits(blocks, final)[0]


def expand(blocks):
    """the bytes the tokens of well-formed blocks stand for"""
    out = bytearray()
    for b in blocks:
        if b["type"] == "stored":
            out += b["data"]
            continue
        for t in b["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                length, dist = t[0], t[1]
                assert isinstance(length, int) and dist <= len(out)
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
Match = collections.namedtuple("Match", "out_pos len dist lit_code_len dist_code_len bits block index")


class Profile:
    def __init__(self):
        self.blocks, self.matches = [], []     # blocks: {"type", "symbols", "stored_len", "start", "lit_code_lens", "dist_code_lens"}


class _Bad(Exception):
    pass


class _Reader:
    def __init__(self, data):
        self.data, self.pos, self.end = data, 0, 8 * len(data)

    def bit(self):
        p = self.pos
        if p >= self.end:
            raise _Bad("input ends")
        self.pos = p + 1
        return self.data[p >> 3] >> (p & 7) & 1

    def bits(self, n):
        v = 0
        for k in range(n):
            v |= self.bit() << k
        return v


def _code_table(lengths, kind):
    """{(length, code): symbol}, after zlib's checks of the set; kind: "codes" (the code-length code), "lens", "dists" """
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    longest = max((l for l in range(16) if count[l]), default=0)
    if longest == 0:
        if kind != "dists":
            raise _Bad("no codes")
        return {}
    left = 1
    for l in range(1, 16):
        left = left * 2 - count[l]
        if left < 0:
            raise _Bad("over-subscribed")
    if left > 0 and (kind == "codes" or longest != 1):
        raise _Bad("incomplete set")
    return {(lengths[s], c): s for s, c in canonical_codes(lengths).items()}


def _symbol(r, table):
    code = 0
    for n in range(1, 16):
        code = code << 1 | r.bit()
        s = table.get((n, code))
        if s is not None:
            return s, n
    raise _Bad("no such code")


def inflate(payload, limit=None):
    """(ok, bytes, Profile); bytes and profile are what was decoded up to the end or the first thing wrong"""
    r, out, prof = _Reader(payload), bytearray(), Profile()
    try:
        final = 0
        while not final:
            final = r.bit()
            btype = r.bits(2)
            block = {"type": ("stored", "fixed", "dynamic", "reserved")[btype], "symbols": 0, "stored_len": None, "start": len(out),
                     "lit_code_lens": collections.Counter(), "dist_code_lens": collections.Counter(), "ended": False}
            prof.blocks.append(block)
            if btype == 3:
                raise _Bad("block type 3")
            if btype == 0:
                r.pos = (r.pos + 7) // 8 * 8
                n, nn = r.bits(16), r.bits(16)
                if n ^ 0xFFFF != nn:
                    raise _Bad("stored lengths")
                at = r.pos >> 3
                if at + n > len(payload):
                    raise _Bad("input ends")
                if limit is not None and len(out) + n > limit:
                    raise _Bad("too many bytes")
                out += payload[at:at + n]
                r.pos += 8 * n
                block["stored_len"] = n
                block["ended"] = True
                continue
            if btype == 1:
                lit_lengths, dist_lengths = FIXED_LIT, FIXED_DIST
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise _Bad("too many symbols")
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = r.bits(3)
                cl_table = _code_table(cl, "codes")
                lengths = []
                while len(lengths) < hlit + hdist:
                    s, _n = _symbol(r, cl_table)
                    if s < 16:
                        lengths.append(s)
                        continue
                    if s == 16:
                        if not lengths:
                            raise _Bad("repeat of nothing")
                        run = [lengths[-1]] * (3 + r.bits(2))
                    else:
                        run = [0] * (3 + r.bits(3) if s == 17 else 11 + r.bits(7))
                    if len(lengths) + len(run) > hlit + hdist:
                        raise _Bad("repeat runs over the end")
                    lengths += run
                lit_lengths, dist_lengths = lengths[:hlit], lengths[hlit:]
                if lit_lengths[EOB] == 0:
                    raise _Bad("no end-of-block code")
            lit_table, dist_table = _code_table(lit_lengths, "lens"), _code_table(dist_lengths, "dists")
            while True:
                first = r.pos
                s, n = _symbol(r, lit_table)
                block["lit_code_lens"][n] += 1
                if s == EOB:
                    block["ended"] = True
                    break
                if s < 256:
                    if limit is not None and len(out) >= limit:
                        raise _Bad("too many bytes")
                    out.append(s)
                    block["symbols"] += 1
                    continue
                if s >= 286:
                    raise _Bad("length symbol 286 / 287")
                length = LENGTH_BASE[s - 257] + r.bits(LENGTH_EXTRA[s - 257])
                d, dn = _symbol(r, dist_table)
                block["dist_code_lens"][dn] += 1
                if d >= 30:
                    raise _Bad("distance symbol 30 / 31")
                dist = DIST_BASE[d] + r.bits(DIST_EXTRA[d])
                if dist > len(out):
                    raise _Bad("distance too far back")
                if limit is not None and len(out) + length > limit:
                    raise _Bad("too many bytes")
                prof.matches.append(Match(len(out), length, dist, n, dn, r.pos - first, len(prof.blocks) - 1, block["symbols"]))
                block["symbols"] += 1
                for _ in range(length):
                    out.append(out[-dist])
        return True, bytes(out), prof
    except _Bad:
        return False, bytes(out), prof

"""The checker of the sorted, tabix-indexed BGZF output, independent of the product code (no import from svtyper_amd):

  (a) parse / table      the per-line rule of the tabix VCF preset restated with split("\\t")
  (b) read_tbi           a reader of the published .tbi layout: gzip.decompress, struct, the fixed header fields checked
  (c) query              a region query as a tabix reader makes it: reg2bins, the linear index, seeks to virtual offsets
  (d) check_structure    what every index of a file has to satisfy, whoever wrote it
  (e) the corpus         lines with what the rule gives for them written down by hand (LINES), whole texts (TEXTS), texts in
                         orders that matter to the sort (ORDERS)

Nothing on the machines the suite runs on reads a .tbi (no htslib, pysam or tabix), so the yardstick is the published format
and this reader; byte equality with `tabix -p vcf` is not claimed anywhere."""
import gzip
import random
import struct

META, BAD, RANGE = 1, 2, 4
TILE = 4096                 # bytes of text per wavefront of the line-table kernels
PAYLOAD = 65280             # bytes of text per BGZF member
TBI_END = 1 << 29
SATURATED = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------ (a) the rule
def parse(line: bytes):
    """one line (with or without its newline) -> (beg, end, chrom_len, flags)"""
    if line.endswith(b"\n"):
        line = line[:-1]
    if line.startswith(b"#"):
        return 0, 0, 0, META
    cols = line.split(b"\t")
    if len(cols) < 8:
        return 0, 0, 0, BAD
    pos = cols[1]
    if not (1 <= len(pos) <= 10) or any(c not in b"0123456789" for c in pos) or int(pos) >= 1 << 31:
        return 0, 0, 0, BAD
    beg = max(int(pos) - 1, 0)
    end = beg + len(cols[3])
    for field in cols[7].split(b";"):
        if field.startswith(b"END=") and field[4:5].isdigit():
            digits = field[4:]
            for k, c in enumerate(digits):
                if c not in b"0123456789":
                    digits = digits[:k]
                    break
            if len(digits) <= 10 and int(digits) > beg:
                end = int(digits)
            break
    return beg, min(end, SATURATED), min(len(cols[0]), SATURATED), RANGE if end > TBI_END else 0


def split_lines(text: bytes):
    """the lines of `text`, newlines kept; the last one may lack it"""
    parts = text.split(b"\n")
    return [p + b"\n" for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def table(text: bytes):
    """[(off, len, beg, end, chrom_len, flags)] per line, in text order"""
    out, at = [], 0
    for line in split_lines(text):
        out.append((at, len(line)) + parse(line))
        at += len(line)
    assert at == len(text)
    return out


def header_count(lines):
    n = 0
    while n < len(lines) and lines[n].startswith(b"#"):
        n += 1
    return n


def sorted_text(text: bytes) -> bytes:
    """the order --sort writes: the header, then the body in stable order by (contig rank, POS)"""
    lines = split_lines(text)
    if lines and not lines[-1].endswith(b"\n"):
        lines[-1] += b"\n"
    h = header_count(lines)
    rank = {}
    for line in lines[:h]:
        if line.startswith(b"##contig=<"):
            for part in line[len(b"##contig=<"):].rstrip(b"\n").rstrip(b">").split(b","):
                if part.startswith(b"ID="):
                    rank.setdefault(part[3:], len(rank))
                    break
    body = lines[h:]
    for line in body:
        rank.setdefault(line.split(b"\t")[0], len(rank))
    body.sort(key=lambda l: (rank[l.split(b"\t")[0]], int(l.split(b"\t")[1])))       # (list.sort is stable)
    return b"".join(lines[:h] + body)


def first_out_of_order(text: bytes):
    """the 1-based number of the first body line a .tbi cannot take as the text stands (a contig that reappears, a beg that
    decreases), or None"""
    lines = split_lines(text)
    seen, cur, last = set(), None, 0
    for k in range(header_count(lines), len(lines)):
        chrom = lines[k].split(b"\t")[0]
        beg = parse(lines[k])[0]
        if chrom != cur:
            if chrom in seen:
                return k + 1
            seen.add(chrom)
            cur = chrom
        elif beg < last:
            return k + 1
        last = beg
    return None


def data_rows(text: bytes):
    """[(contig, beg, end with an empty REF's base, line)] of the body, in text order"""
    lines = split_lines(text)
    rows = []
    for line in lines[header_count(lines):]:
        b, e, _, _ = parse(line)
        rows.append((line.split(b"\t")[0], b, max(e, b + 1), line))
    return rows


def scan(rows, contig: bytes, beg: int, end: int):
    """brute force over data_rows(text): the data lines of `contig` whose interval overlaps [beg, end), in text order"""
    return [line for chrom, b, e, line in rows if chrom == contig and b < end and e > beg]


# ------------------------------------------------------------------------------------------ (b) the .tbi reader
def reg2bin(beg: int, end: int) -> int:
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg: int, end: int):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def read_tbi(data: bytes):
    """the bytes of a .tbi file -> {"names": [...], "refs": [{"bins": {bin: [(beg, end)]}, "ioff": [...], "pseudo": ... or None}]}"""
    raw = gzip.decompress(data)
    assert data[-28:] == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"), "no BGZF EOF member"
    assert raw[:4] == b"TBI\1"
    n_ref, fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<8i", raw, 4)
    assert (fmt, col_seq, col_beg, col_end, meta, skip) == (2, 1, 2, 0, ord("#"), 0)
    at = 36
    blob = raw[at:at + l_nm]
    at += l_nm
    names = blob.split(b"\0")[:-1] if l_nm else []
    assert len(names) == n_ref and (not l_nm or blob.endswith(b"\0")) and len(set(names)) == n_ref
    refs = []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", raw, at)
        at += 4
        bins, pseudo = {}, None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", raw, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", raw, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            assert b not in bins and (b < 37449 or b == 37450)
            if b == 37450:
                assert n_chunk == 2
                pseudo = chunks
            else:
                bins[b] = chunks
        n_intv, = struct.unpack_from("<i", raw, at)
        at += 4
        ioff = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
        at += 8 * n_intv
        refs.append({"bins": bins, "ioff": ioff, "pseudo": pseudo})
    assert at == len(raw), "bytes behind the last contig"
    return {"names": names, "refs": refs}


def build_tbi(text: bytes, member_off, payload=PAYLOAD) -> bytes:
    """The uncompressed bytes of a .tbi for sorted, indexable `text` whose payload k (text bytes [k * payload, ...)) lies in the
    member at file offset member_off[k]; member_off[-1] is where the members end.  A loop over the lines in plain Python: the
    restatement of the fold and the CPU yardstick of tools/tabix_ab.py."""
    n_members = len(member_off) - 1

    def voff(x):
        k = x // payload
        return member_off[n_members] << 16 if k >= n_members else member_off[k] << 16 | (x - k * payload)

    lines = split_lines(text)
    at = sum(len(l) for l in lines[:header_count(lines)])
    refs, cur, last_bin = [], None, None
    for line in lines[header_count(lines):]:
        b, e, _, flags = parse(line)
        assert flags == 0
        e = max(e, b + 1)
        name = line.split(b"\t")[0]
        if cur is None or cur["name"] != name:
            assert all(r["name"] != name for r in refs)
            cur = {"name": name, "bins": {}, "ioff": [], "lines": 0, "first": voff(at), "last": 0}
            refs.append(cur)
            last_bin = None
        s, t = voff(at), voff(at + len(line))
        bin_ = reg2bin(b, e)
        if bin_ == last_bin:
            cur["bins"][bin_][-1][1] = t
        else:
            cur["bins"].setdefault(bin_, []).append([s, t])
        last_bin = bin_
        while len(cur["ioff"]) <= (e - 1) >> 14:
            cur["ioff"].append(None)
        for w in range(b >> 14, ((e - 1) >> 14) + 1):
            cur["ioff"][w] = s if cur["ioff"][w] is None else min(cur["ioff"][w], s)
        cur["lines"] += 1
        cur["last"] = t
        at += len(line)
    names = b"".join(r["name"] + b"\0" for r in refs)
    out = [b"TBI\1", struct.pack("<8i", len(refs), 2, 1, 2, 0, ord("#"), 0, len(names)), names]
    for r in refs:
        out.append(struct.pack("<i", len(r["bins"]) + 1))
        for bin_ in sorted(r["bins"]):
            out.append(struct.pack("<Ii", bin_, len(r["bins"][bin_])))
            out.extend(struct.pack("<QQ", *c) for c in r["bins"][bin_])
        out.append(struct.pack("<IiQQQQ", 37450, 2, r["first"], r["last"], r["lines"], 0))
        for w in range(len(r["ioff"]) - 2, -1, -1):
            if r["ioff"][w] is None:
                r["ioff"][w] = r["ioff"][w + 1]
        out.append(struct.pack("<i%dQ" % len(r["ioff"]), len(r["ioff"]), *r["ioff"]))
    return b"".join(out)


# ------------------------------------------------------------------------------------------ (c) the query
class Members:
    """a BGZF file's members by file offset"""

    def __init__(self, data: bytes):
        self.payload, self.next, self.order = {}, {}, []
        at = 0
        while at < len(data):
            assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\0"
            size = struct.unpack_from("<H", data, at + 16)[0] + 1
            self.payload[at] = gzip.decompress(data[at:at + size])
            self.next[at] = at + size
            self.order.append(at)
            at += size
        assert at == len(data)
        self.end = at
        assert self.order and self.payload[self.order[-1]] == b"" and self.next[self.order[-1]] - self.order[-1] == 28, "no BGZF EOF member"

    def text(self) -> bytes:
        return b"".join(self.payload[at] for at in self.order)

    def valid(self, voff: int) -> bool:
        at, within = voff >> 16, voff & 0xFFFF
        return (at in self.payload and within <= len(self.payload[at])) or (at == self.end and within == 0)

    def canonical(self, voff: int) -> int:
        """the same place named by the member that holds its next byte"""
        at, within = voff >> 16, voff & 0xFFFF
        while at in self.payload and within == len(self.payload[at]):
            at, within = self.next[at], 0
        return at << 16 | within

    def read(self, beg: int, end: int) -> bytes:
        """the inflated bytes from virtual offset beg to virtual offset end"""
        beg, end = self.canonical(beg), self.canonical(end)
        out = []
        at, within = beg >> 16, beg & 0xFFFF
        while at << 16 | within < end:
            stop = end & 0xFFFF if at == end >> 16 else len(self.payload[at])
            out.append(self.payload[at][within:stop])
            if at == end >> 16:
                break
            at, within = self.next[at], 0
        return b"".join(out)

    def voff_of(self, pos: int) -> int:
        """the canonical virtual offset of text position `pos`; the text's end is the end of the members in front of the EOF member"""
        for at in self.order:
            size = len(self.payload[at])
            if pos < size:
                return at << 16 | pos
            pos -= size
        assert pos == 0
        return self.end << 16

    def line_places(self):
        """the canonical virtual offset of every line's start, in text order, and of the text's end"""
        places, pos = [], 0
        starts = iter(self.order)
        at, left = next(starts), 0
        base = 0                    # text position of payload `at`
        for line in split_lines(self.text()):
            while pos - base >= len(self.payload[at]):
                base += len(self.payload[at])
                at = next(starts)
            places.append(at << 16 | (pos - base))
            pos += len(line)
        return places, self.end << 16


def query(vcf_gz: bytes, tbi, contig: bytes, beg: int, end: int, members=None):
    """the data lines of `contig` that overlap [beg, end), found through the index alone"""
    if contig not in tbi["names"] or end <= beg:
        return []
    m = members or Members(vcf_gz)
    ref = tbi["refs"][tbi["names"].index(contig)]
    w = beg >> 14
    min_off = ref["ioff"][w] if w < len(ref["ioff"]) else (ref["ioff"][-1] if ref["ioff"] else 0)
    chunks = sorted(c for b in reg2bins(beg, min(end, TBI_END)) for c in ref["bins"].get(b, ()) if c[1] > min_off)
    out = []
    for c_beg, c_end in chunks:
        for line in split_lines(m.read(c_beg, c_end)):
            b, e, _, flags = parse(line)
            assert flags == 0 and line.split(b"\t")[0] == contig, "a chunk holds a line of another contig"
            if b < end and max(e, b + 1) > beg:
                out.append(line)
    return out


# ------------------------------------------------------------------------------------------ (d) structure
def check_structure(vcf_gz: bytes, tbi, members=None):
    m = members or Members(vcf_gz)
    lines = split_lines(m.text())
    place, text_end = m.line_places()
    starts = set(place) | {text_end}
    data_lines = [(j, parse(lines[j])) for j in range(header_count(lines), len(lines))]
    contigs = []
    for j, (b, e, _, flags) in data_lines:
        assert flags == 0, "line %d is not indexable" % (j + 1)
        name = lines[j].split(b"\t")[0]
        if name not in contigs:
            contigs.append(name)
    assert tbi["names"] == contigs, "the names are the contigs in order of first appearance"
    for tid, ref in enumerate(tbi["refs"]):
        all_chunks = []
        for b, chunks in ref["bins"].items():
            for c_beg, c_end in chunks:
                assert m.valid(c_beg) and m.valid(c_end) and m.canonical(c_beg) < m.canonical(c_end), "an empty or misplaced chunk"
                assert m.canonical(c_beg) in starts and m.canonical(c_end) in starts, "a chunk cuts a line"
                all_chunks.append((m.canonical(c_beg), m.canonical(c_end), b))
        mine = [(j, p) for j, p in data_lines if lines[j].split(b"\t")[0] == tbi["names"][tid]]
        for j, (b, e, _, _) in mine:
            e = max(e, b + 1)
            holders = [c for c in all_chunks if c[0] <= place[j] < c[1]]
            assert len(holders) == 1 and holders[0][2] == reg2bin(b, e), "line %d: %r, wanted bin %d" % (j + 1, holders, reg2bin(b, e))
            for w in range(b >> 14, ((e - 1) >> 14) + 1):
                assert w < len(ref["ioff"]) and m.canonical(ref["ioff"][w]) <= place[j], "line %d: ioff[%d] lies behind it" % (j + 1, w)
        if ref["pseudo"] is not None:
            assert ref["pseudo"][1] == (len(mine), 0)
            assert m.canonical(ref["pseudo"][0][0]) == place[mine[0][0]]


def check_queries(vcf_gz: bytes, tbi, regions, members=None):
    m = members or Members(vcf_gz)
    rows = data_rows(m.text())
    for contig, beg, end in regions:
        assert query(vcf_gz, tbi, contig, beg, end, m) == scan(rows, contig, beg, end), (contig, beg, end)


def regions_of(text: bytes, seed=7, n_random=200):
    """every interval edge of the text +-1 as a one-base and as an open query, and seeded random regions"""
    lines = split_lines(text)
    regions, contigs, top = [], [], 1
    for line in lines[header_count(lines):]:
        b, e, _, flags = parse(line)
        if flags:
            continue
        chrom = line.split(b"\t")[0]
        if chrom not in contigs:
            contigs.append(chrom)
        top = max(top, e)
        for edge in (b, max(e, b + 1)):
            for x in (edge - 1, edge, edge + 1):
                if 0 <= x < TBI_END:
                    regions.append((chrom, x, x + 1))
                    regions.append((chrom, max(x - 20000, 0), x))
    regions = sorted(set(regions))
    rng = random.Random(seed)
    for _ in range(n_random if contigs else 0):
        beg = rng.randrange(0, min(top + 20000, TBI_END - 1))
        regions.append((rng.choice(contigs + [b"nowhere"]), beg, min(beg + rng.choice((1, 100, 20000, 1 << 22)), TBI_END)))
    return regions


# ------------------------------------------------------------------------------------------ (e) the corpus
HEADER = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\n"


def vcf_line(chrom, pos, ident, ref="A", alt="T", info=".", more=("GT", "0/1"), newline=True):
    cols = [str(chrom), str(pos), ident, ref, alt, ".", "PASS", info] + list(more)
    return "\t".join(cols).encode() + (b"\n" if newline else b"")


# name -> (line, (beg, end, flags)): what the rule gives, written down by hand
LINES = {
    "end_first": (vcf_line(1, 100, "a", info="END=500;SVTYPE=DEL"), (99, 500, 0)),
    "end_after_semicolon": (vcf_line(1, 100, "b", info="SVTYPE=DEL;END=600"), (99, 600, 0)),
    "no_end": (vcf_line(1, 100, "c", ref="ACGT", info="SVTYPE=DEL"), (99, 103, 0)),
    "ciend_alone": (vcf_line(1, 100, "d", info="CIEND=-10,10"), (99, 100, 0)),
    "ciend_before_end": (vcf_line(1, 100, "e", info="CIEND=-10,10;END=700"), (99, 700, 0)),
    "xend": (vcf_line(1, 100, "f", info="XEND=900;SVTYPE=DEL"), (99, 100, 0)),
    "end2": (vcf_line(1, 100, "g", info="END2=900"), (99, 100, 0)),
    "end_is_beg": (vcf_line(1, 100, "h", info="END=99"), (99, 100, 0)),
    "end_is_beg_plus_1": (vcf_line(1, 100, "i", ref="ACG", info="END=100"), (99, 100, 0)),
    "end_not_a_number": (vcf_line(1, 100, "j", info="END=abc"), (99, 100, 0)),
    "end_negative": (vcf_line(1, 100, "k", info="END=-5"), (99, 100, 0)),
    "end_negative_then_real": (vcf_line(1, 100, "k2", info="END=-5;END=300"), (99, 300, 0)),
    "end_11_digits": (vcf_line(1, 100, "l", info="END=12345678901"), (99, 100, 0)),
    "end_11_digits_then_real": (vcf_line(1, 100, "l2", info="END=12345678901;END=300"), (99, 100, 0)),
    "end_first_decides": (vcf_line(1, 100, "m", info="END=200;END=300"), (99, 200, 0)),
    "end_with_tail": (vcf_line(1, 100, "m2", info="END=250x"), (99, 250, 0)),
    "end_bare": (vcf_line(1, 100, "m3", info="END"), (99, 100, 0)),
    "info_dot": (vcf_line(1, 100, "n", info="."), (99, 100, 0)),
    "pos_0": (vcf_line(1, 0, "o"), (0, 1, 0)),
    "pos_1": (vcf_line(1, 1, "p"), (0, 1, 0)),
    "pos_10_digits": (vcf_line(1, "0000000100", "p2"), (99, 100, 0)),
    "ref_300": (vcf_line(1, 1000, "q", ref="ACGT" * 75), (999, 1299, 0)),
    "ref_empty": (vcf_line(1, 1000, "q2", ref=""), (999, 999, 0)),
    "bnd_after": (vcf_line(1, 2000, "r_1", ref="N", alt="N]2:3000]", info="SVTYPE=BND;MATEID=r_2"), (1999, 2000, 0)),
    "bnd_before": (vcf_line(2, 3000, "r_2", ref="N", alt="[1:2000[N", info="SVTYPE=BND;MATEID=r_1;END=1"), (2999, 3000, 0)),
    "eight_columns": (vcf_line(1, 100, "s", more=()), (99, 100, 0)),
    "eight_columns_end": (vcf_line(1, 100, "s2", info="END=150", more=()), (99, 150, 0)),
    "seven_columns": (b"1\t100\tt\tA\tT\t.\tPASS\n", (0, 0, BAD)),
    "empty": (b"\n", (0, 0, BAD)),
    "pos_12a": (vcf_line(1, "12a", "u"), (0, 0, BAD)),
    "pos_empty": (vcf_line(1, "", "u2"), (0, 0, BAD)),
    "pos_11_digits": (vcf_line(1, "00000000100", "u3"), (0, 0, BAD)),
    "pos_2_31": (vcf_line(1, 1 << 31, "u4"), (0, 0, BAD)),
    "pos_negative": (vcf_line(1, -5, "u5"), (0, 0, BAD)),
    "meta": (b"##INFO=<ID=END,Number=1>\n", (0, 0, META)),
    "end_2_29": (vcf_line(1, 100, "v", info="END=%d" % (1 << 29)), (99, 1 << 29, 0)),
    "end_2_29_plus_1": (vcf_line(1, 100, "w", info="END=%d" % ((1 << 29) + 1)), (99, (1 << 29) + 1, RANGE)),
    "end_10_digits": (vcf_line(1, 100, "w2", info="END=9999999999"), (99, SATURATED, RANGE)),
    "pos_top": (vcf_line(1, (1 << 31) - 1, "w3"), ((1 << 31) - 2, (1 << 31) - 1, RANGE)),
    "two_bytes": (b"x\n", (0, 0, BAD)),
}
for _shift in (14, 17, 20, 23, 26):     # beg and end on both sides of every bin edge
    _edge = 1 << _shift
    LINES["edge%d_ends_at" % _shift] = (vcf_line(1, _edge - 9, "z", info="END=%d" % _edge), (_edge - 10, _edge, 0))
    LINES["edge%d_crosses" % _shift] = (vcf_line(1, _edge - 9, "z", info="END=%d" % (_edge + 1)), (_edge - 10, _edge + 1, 0))
    LINES["edge%d_last_base" % _shift] = (vcf_line(1, _edge, "z"), (_edge - 1, _edge, 0))
    LINES["edge%d_first_base" % _shift] = (vcf_line(1, _edge + 1, "z"), (_edge, _edge + 1, 0))
    LINES["edge%d_begins_at" % _shift] = (vcf_line(1, _edge + 1, "z", info="END=%d" % (_edge + 500)), (_edge, _edge + 500, 0))


def _indexable(names):
    return [LINES[n][0] for n in names if LINES[n][1][2] == 0]


def _by_pos(lines):
    return sorted(lines, key=lambda l: (l.split(b"\t")[0] != b"1", int(l.split(b"\t")[1])))


def _long(pos, ident, size):
    """a line of `size` bytes: sample columns, the first eight columns short"""
    head = vcf_line(1, pos, ident, info="END=%d" % (pos + 50), more=("GT",), newline=False)
    fill = size - len(head) - 1
    return head + b"\t" + (b"0/1\t" * (fill // 4 + 1))[:fill - 1] + b"\n"


def _tile_text(offset):
    """a text whose line `x` ends with its newline as byte TILE - 1 + offset: the last byte of a tile (0) or the first of the next (1)"""
    lines = [vcf_line(1, 10, "t1"), vcf_line(1, 20, "t2")]
    used = len(HEADER) + sum(map(len, lines))
    pad = vcf_line(1, 30, "x", more=("GT", ""), newline=False)
    want = TILE + offset - used
    lines.append(pad + b"0" * (want - len(pad) - 1) + b"\n")
    lines.append(vcf_line(1, 40, "t3"))
    lines.append(vcf_line(1, 50, "t4"))
    text = HEADER + b"".join(lines)
    assert text[TILE - 1 + offset:TILE + offset] == b"\n"
    return text


def _payload_text():
    """a text of exactly PAYLOAD bytes: its end is the end of its only member"""
    front = HEADER + vcf_line(1, 5, "s")
    head = vcf_line(1, 900000, "p", more=("GT", "."), newline=False)
    return front + head + b"." * (PAYLOAD - len(front) - len(head) - 1) + b"\n"


# whole texts inside the envelope (sorted, indexable): name -> text
TEXTS = {
    "every_indexable_line": HEADER + b"".join(_by_pos(_indexable(sorted(LINES)))),
    "no_data_lines": HEADER,
    "nothing": b"",
    "last_line_without_newline": HEADER + vcf_line(1, 100, "a") + vcf_line(1, 200, "b", info="END=300", newline=False),
    "one_line_without_newline": vcf_line(1, 100, "a", newline=False),
    "spans_two_members": HEADER + vcf_line(1, 5, "s") + _long(10, "long2", 70000) + vcf_line(1, 80, "e"),
    "spans_three_members": HEADER + vcf_line(1, 5, "s") + _long(10, "long3", 140000) + vcf_line(1, 80, "e") + _long(90, "again", 70000),
    "newline_ends_a_tile": _tile_text(0),
    "newline_begins_a_tile": _tile_text(1),
    "many_short_lines": HEADER + b"".join(vcf_line(1 + k // 110, 10 + 3 * (k % 110), "n%d" % k, more=()) for k in range(330)),
    "exactly_one_payload": _payload_text(),
}
# texts of lines only, for the line table alone (nothing here is written or indexed): BAD, META and RANGE lines among data lines
TABLE_TEXTS = dict(TEXTS)
TABLE_TEXTS.update({
    "every_line": b"".join(LINES[n][0] for n in sorted(LINES)),
    "two_byte_lines": b"x\n" * 3000 + b"y",
    "newlines_only": b"\n" * 5000,
    "no_newline_at_all": b"z" * 9000,
})

CONTIG_HEADER = b"##fileformat=VCFv4.2\n##contig=<ID=chrB,length=1000>\n##contig=<ID=chrA,length=1000>\n##contig=<length=5,ID=chrC>\n" + HEADER.split(b"\n", 1)[1]
_sorted_body = [vcf_line("chrB", 5, "b1"), vcf_line("chrB", 9, "b2"), vcf_line("chrA", 1, "a1"), vcf_line("chrA", 70, "a2"), vcf_line("chrC", 3, "c1")]
# orders for the sort: name -> text (all sortable; which of them a .tbi can take unsorted is first_out_of_order's to say)
ORDERS = {
    "already_sorted": CONTIG_HEADER + b"".join(_sorted_body),
    "reversed": CONTIG_HEADER + b"".join(reversed(_sorted_body)),
    "equal_keys": CONTIG_HEADER + b"".join(vcf_line("chrA", 7, "tie%d" % k, ref="A" * (5 - k)) for k in range(5)) + vcf_line("chrB", 7, "front"),
    "declared_order_differs": CONTIG_HEADER + vcf_line("chrA", 5, "a") + vcf_line("chrC", 5, "c") + vcf_line("chrB", 5, "b"),
    "undeclared_contig": CONTIG_HEADER + vcf_line("zz", 5, "z1") + vcf_line("chrA", 5, "a") + vcf_line("zz", 2, "z2") + vcf_line("chrB", 1, "b"),
    "contig_reappears": HEADER + vcf_line(2, 5, "x1") + vcf_line(3, 5, "y") + vcf_line(2, 1, "x2") + vcf_line(15, 4, "w"),
    "pos_0_and_1": HEADER + vcf_line(1, 1, "one") + vcf_line(1, 0, "zero") + vcf_line(1, 1, "one_again"),
    "pos_decreases": HEADER + vcf_line(1, 500, "late") + vcf_line(1, 20, "early", newline=False),
    "bnd_mates_part": HEADER + LINES["bnd_after"][0] + LINES["bnd_before"][0] + vcf_line(1, 2500, "between"),
}

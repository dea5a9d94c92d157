"""The CSI index of the sorted `-w` BAM and the sorted VCF: a plain-Python restatement of the fold, an independent CSI reader, the
new inputs, and checks that compare region queries through the index with a linear scan.  Nothing here imports svtyper_amd.

The fold, restated: the scheme is (14, depth) with the smallest depth >= 5 whose 2^(14 + 3 depth) covers the file
(BAM: the header's longest reference; VCF: the largest end among the body lines).  Per reference, in file order: a record goes
into the smallest bin that holds [beg, max(end, beg + 1)); a run of consecutive records with one bin is one chunk from the
first record's start to the last record's end; the loffset of a bin is the start of the first record of the reference whose
running maximum of `end` lies behind the bin's first position; the pseudo-bin carries (first start, last end) and (mapped,
unmapped).  Byte equality with htslib's .csi is not claimed anywhere: what is asked of an index is that every query through
it finds what the scan finds."""
import random
import struct
import zlib

import baicases as B
import tbxcases as T

MIN_SHIFT = 14
SATURATED = 0xFFFFFFFF
EOF = B.EOF


# ------------------------------------------------------------------------------------------ the scheme
def depth_for(max_end):
    d = 5
    while 1 << (MIN_SHIFT + 3 * d) < max_end:
        d += 1
    return d


def level_first(l):
    return ((1 << (3 * l)) - 1) // 7


def reg2bin(beg, end, depth):
    end -= 1
    shift = MIN_SHIFT
    for l in range(depth, 0, -1):
        if beg >> shift == end >> shift:
            return level_first(l) + (beg >> shift)
        shift += 3
    return 0


def reg2bins(beg, end, depth):
    end -= 1
    bins = []
    for l in range(depth + 1):
        shift = MIN_SHIFT + 3 * (depth - l)
        bins.extend(range(level_first(l) + (beg >> shift), level_first(l) + (end >> shift) + 1))
    return bins


def bin_start(b, depth):
    l = 0
    while l < depth and level_first(l + 1) <= b:
        l += 1
    return (b - level_first(l)) << (MIN_SHIFT + 3 * (depth - l))


def pseudo_bin(depth):
    return level_first(depth + 1) + 1


# ------------------------------------------------------------------------------------------ the fold
def fold(depth, aux, n_ref, placed, no_coor):
    """the uncompressed bytes of a CSI.  `placed`: (tid, beg, end, s, e, unmapped) per record with a coordinate, in file order"""
    limit = 1 << (MIN_SHIFT + 3 * depth)
    refs = [dict(bins={}, last_bin=None, ends=[], n=0, unmapped=0, first=0, last=0) for _ in range(n_ref)]
    for tid, beg, end, s, e, unmapped in placed:
        end = max(end, beg + 1)
        assert end <= limit and end != SATURATED, "the scheme does not cover the record"
        r = refs[tid]
        b = reg2bin(beg, end, depth)
        if b == r["last_bin"]:
            r["bins"][b][-1][1] = e
        else:
            r["bins"].setdefault(b, []).append([s, e])
        r["last_bin"] = b
        r["ends"].append((max(end, r["ends"][-1][0]) if r["ends"] else end, s))
        if not r["n"]:
            r["first"] = s
        r["last"] = e
        r["n"] += 1
        r["unmapped"] += bool(unmapped)
    out = [b"CSI\1", struct.pack("<iii", MIN_SHIFT, depth, len(aux)), aux, struct.pack("<i", n_ref)]
    for r in refs:
        if not r["n"]:
            out.append(struct.pack("<i", 0))
            continue
        out.append(struct.pack("<i", len(r["bins"]) + 1))
        for b in sorted(r["bins"]):
            start = bin_start(b, depth)
            loffset = next(s for top, s in r["ends"] if top > start)
            out.append(struct.pack("<IQi", b, loffset, len(r["bins"][b])))
            out.extend(struct.pack("<QQ", *c) for c in r["bins"][b])
        out.append(struct.pack("<IQiQQQQ", pseudo_bin(depth), 0, 2, r["first"], r["last"], r["n"] - r["unmapped"], r["unmapped"]))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def l_ref_max(header):
    """the longest reference of a BAM header"""
    l_text = struct.unpack_from("<i", header, 4)[0]
    at, top = 12 + l_text, 0
    for _ in range(struct.unpack_from("<i", header, 8 + l_text)[0]):
        l_name = struct.unpack_from("<i", header, at)[0]
        top = max(top, struct.unpack_from("<i", header, at + 4 + l_name)[0])
        at += 8 + l_name
    return top


def build_csi_bam(w):
    """the uncompressed .csi of the baicases.Written file `w`"""
    placed, no_coor = [], 0
    for raw, at, (_key, tid, beg, end, flags) in zip(w.records, w.offsets, w.rows):
        assert not flags & B.BAD
        if flags & B.NO_COOR:
            no_coor += 1
            continue
        placed.append((tid, beg, end, w.voffset(at), w.voffset(at + len(raw)), flags & B.UNMAPPED))
    return fold(depth_for(l_ref_max(w.header)), b"", w.n_ref, placed, no_coor)


def vcf_depth(text):
    rows = T.data_rows(text)
    return depth_for(max([e for _c, _b, e, _l in rows] or [0]))


def build_csi_vcf(text, member_off, payload=T.PAYLOAD):
    """the uncompressed .csi of sorted `text` whose payload k lies in the member at file offset member_off[k]"""
    n_members = len(member_off) - 1

    def voff(x):
        k = x // payload
        return member_off[n_members] << 16 if k >= n_members else member_off[k] << 16 | (x - k * payload)

    lines = T.split_lines(text)
    at = sum(len(l) for l in lines[:T.header_count(lines)])
    names, placed = [], []
    for line in lines[T.header_count(lines):]:
        b, e, _, flags = T.parse(line)
        assert not flags & (T.META | T.BAD)
        name = line.split(b"\t")[0]
        if not names or names[-1] != name:
            assert name not in names
            names.append(name)
        placed.append((len(names) - 1, b, e, voff(at), voff(at + len(line)), False))
        at += len(line)
    blob = b"".join(n + b"\0" for n in names)
    aux = struct.pack("<7i", 2, 1, 2, 0, ord("#"), 0, len(blob)) + blob
    return fold(vcf_depth(text), aux, len(names), placed, 0)


# ------------------------------------------------------------------------------------------ the reader
def inflate(data):
    """the payload of the BGZF file `data`: every member inflated here, its CRC and ISIZE checked, the EOF member required"""
    out, at = [], 0
    assert data.endswith(EOF), "no BGZF EOF member"
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\0", "not a BGZF member at %d" % at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        payload = zlib.decompress(data[at + 18:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert zlib.crc32(payload) & 0xFFFFFFFF == crc and len(payload) == isize
        out.append(payload)
        at += size
    return b"".join(out)


def read_csi(raw):
    """{"depth", "aux", "refs": [{"bins": {bin: (loffset, [(beg, end)])}, "pseudo": None | [(..), (..)]}], "no_coor"}; all of `raw` is used"""
    assert raw[:4] == b"CSI\1", "no CSI magic"
    min_shift, depth, l_aux = struct.unpack_from("<iii", raw, 4)
    assert min_shift == MIN_SHIFT and 5 <= depth <= 6 and l_aux >= 0
    aux = raw[16:16 + l_aux]
    at = 16 + l_aux
    n_ref = struct.unpack_from("<i", raw, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", raw, at)[0]
        at += 4
        bins, pseudo, last = {}, None, -1
        for _ in range(n_bin):
            b, loffset, n_chunk = struct.unpack_from("<IQi", raw, at)
            at += 16
            chunks = [struct.unpack_from("<QQ", raw, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            assert b > last, "the bins do not rise"
            last = b
            if b == pseudo_bin(depth):
                assert n_chunk == 2 and loffset == 0
                pseudo = chunks
            else:
                assert b < pseudo_bin(depth) - 1 and n_chunk > 0
                bins[b] = (loffset, chunks)
        assert (pseudo is None) == (n_bin == 0), "a reference with records has the pseudo-bin, one without has n_bin = 0"
        refs.append(dict(bins=bins, pseudo=pseudo))
    no_coor = struct.unpack_from("<Q", raw, at)[0]
    assert at + 8 == len(raw), "bytes behind n_no_coor, or none of it"
    return dict(depth=depth, aux=aux, refs=refs, no_coor=no_coor)


def names_of(aux):
    """the contig names of a VCF's aux block"""
    fmt, col_seq, col_beg, col_end, meta, skip, l_nm = struct.unpack_from("<7i", aux, 0)
    assert (fmt, col_seq, col_beg, col_end, meta, skip) == (2, 1, 2, 0, ord("#"), 0) and len(aux) == 28 + l_nm
    blob = aux[28:]
    assert not l_nm or blob.endswith(b"\0")
    return blob.split(b"\0")[:-1] if l_nm else []


def min_offset(ref, beg, depth):
    """an offset no record overlapping [beg, ...) lies in front of, as htslib's iterator finds it: the loffset of beg's leaf if the
    reference has that bin, else of the nearest sibling in front, else -- from the first child -- of the parent, and so on up"""
    b = level_first(depth) + (beg >> MIN_SHIFT)
    while b:
        if b in ref["bins"]:
            return ref["bins"][b][0]
        parent = (b - 1) >> 3
        b = b - 1 if b > (parent << 3) + 1 else parent
    return ref["bins"][0][0] if 0 in ref["bins"] else 0


# ------------------------------------------------------------------------------------------ BAM: structure and queries
def check_structure(csi, w):
    """`csi` (read_csi) against the Written file `w`"""
    depth = csi["depth"]
    assert depth == depth_for(l_ref_max(w.header)) and csi["aux"] == b"" and len(csi["refs"]) == w.n_ref
    starts = set(w.offsets)
    assert csi["no_coor"] == sum(1 for r in w.rows if r[4] & B.NO_COOR)
    for tid, ref in enumerate(csi["refs"]):
        mine = [(r, at, len(raw)) for r, at, raw in zip(w.rows, w.offsets, w.records) if r[1] == tid and not r[4] & B.NO_COOR]
        if not mine:
            assert not ref["bins"] and ref["pseudo"] is None
            continue
        held = []
        for b, (loffset, chunks) in ref["bins"].items():
            last_end = 0
            for beg, end in chunks:
                assert beg < end and beg >= last_end, "chunks of bin %d do not ascend" % b
                last_end = end
                pb, pe = w.position(beg), w.position(end)
                assert pb in starts and (pe in starts or pe == len(w.stream)), "a chunk of bin %d cuts a record" % b
                held.append((pb, pe, b))
            # the loffset: a record start, and no record overlapping a position at or behind the bin's start lies in front of it
            at = w.position(loffset)
            assert at in starts
            start = bin_start(b, depth)
            assert all(r_at >= at for (r, r_at, _n) in mine if max(r[3], r[2] + 1) > start), "bin %d: a record in front of its loffset" % b
            assert any(r_at == at and max(r[3], r[2] + 1) > start for (r, r_at, _n) in mine), "bin %d: its loffset overlaps nothing behind" % b
        for r, at, _n in mine:
            holders = [h for h in held if h[0] <= at < h[1]]
            want = reg2bin(r[2], max(r[3], r[2] + 1), depth)
            assert len(holders) == 1 and holders[0][2] == want, "record at %d: %r, wanted bin %d" % (at, holders, want)
        unmapped = sum(1 for r, _at, _n in mine if r[4] & B.UNMAPPED)
        (first, last), counts = ref["pseudo"]
        assert counts == (len(mine) - unmapped, unmapped)
        assert w.position(first) == mine[0][1] and w.position(last) == mine[-1][1] + mine[-1][2]


def scan(w, tid, beg, end):
    return [at for (_key, t, b, e, flags), at in zip(w.rows, w.offsets) if t == tid and not flags & B.NO_COOR and b < end and max(e, b + 1) > beg]


def query(csi, w, tid, beg, end):
    """the record starts the index leads to for [beg, end) on `tid`"""
    ref, depth = csi["refs"][tid], csi["depth"]
    limit = 1 << (MIN_SHIFT + 3 * depth)
    if beg >= limit or ref["pseudo"] is None:
        return []
    floor = min_offset(ref, beg, depth)
    found = set()
    index_of = {at: i for i, at in enumerate(w.offsets)}
    for b in reg2bins(beg, min(end, limit), depth):
        for cb, ce in ref["bins"].get(b, (0, ()))[1]:
            if ce <= floor:
                continue
            i, stop = index_of[w.position(cb)], w.position(ce)
            while i < len(w.offsets) and w.offsets[i] < stop:
                _key, t, rb, re_, flags = w.rows[i]
                if t == tid and not flags & B.NO_COOR and rb < end and max(re_, rb + 1) > beg and w.offsets[i] >= w.position(floor):
                    found.add(w.offsets[i])
                i += 1
    return sorted(found)


def regions(w, seed=1):
    """(tid, beg, end): every leaf and bin edge next to a record, +-1, at every level of depth 6, and 200 seeded random ones"""
    out = set()
    rnd = random.Random(seed)
    rows = [r for r in w.rows if not r[4] & (B.NO_COOR | B.BAD)]
    top_of = 1 << 32
    for _key, tid, beg, end, _flags in rows:
        end = max(end, beg + 1)
        for shift in (14, 17, 20, 23, 26, 29):
            for edge in {beg >> shift << shift, (beg >> shift) + 1 << shift, (end - 1) >> shift << shift, ((end - 1) >> shift) + 1 << shift}:
                for lo in (edge - 1, edge, edge + 1):
                    if 0 <= lo < top_of:
                        out.add((tid, lo, lo + 1))
                        out.add((tid, max(lo - 100, 0), lo + 1))
        out.add((tid, beg, end))
        out.add((tid, max(beg - 1, 0), beg))
        out.add((tid, end, end + 1))
    if len(out) > 1000:
        out = set(rnd.sample(sorted(out), 1000))
    tids = sorted({r[1] for r in rows}) or [0]
    top = max([r[3] for r in rows] or [1]) + 20000
    more = set()
    while len(more) < 200:
        tid, lo = rnd.choice(tids), rnd.randrange(0, top)
        more.add((tid, lo, lo + rnd.choice((1, 10, 1000, 20000, 1 << 18, 1 << 27))))
    return sorted(out | more)


def check_queries(csi, w, seed=1):
    n = 0
    for tid, beg, end in regions(w, seed):
        assert query(csi, w, tid, beg, end) == scan(w, tid, beg, end), "region %d:%d-%d" % (tid, beg, end)
        n += 1
    return n


# ------------------------------------------------------------------------------------------ VCF: queries
def query_vcf(csi, m, contig, beg, end):
    """the data lines of `contig` that overlap [beg, end), found through the index alone; `m`: tbxcases.Members of the .vcf.gz"""
    names, depth = names_of(csi["aux"]), csi["depth"]
    limit = 1 << (MIN_SHIFT + 3 * depth)
    if contig not in names or end <= beg or beg >= limit:
        return []
    ref = csi["refs"][names.index(contig)]
    floor = m.canonical(min_offset(ref, beg, depth))
    chunks = sorted(c for b in reg2bins(beg, min(end, limit), depth) for c in ref["bins"].get(b, (0, ()))[1] if m.canonical(c[1]) > floor)
    out = []
    for c_beg, c_end in chunks:
        for line in T.split_lines(m.read(max(m.canonical(c_beg), floor), c_end)):
            b, e, _, flags = T.parse(line)
            assert not flags & (T.META | T.BAD) and line.split(b"\t")[0] == contig, "a chunk holds a line of another contig"
            if b < end and max(e, b + 1) > beg:
                out.append(line)
    return out


def regions_vcf(text, seed=7, n_random=200):
    """tbxcases.regions_of without the 2^29 ceiling"""
    lines = T.split_lines(text)
    out, contigs, top = [], [], 1
    for line in lines[T.header_count(lines):]:
        b, e, _, flags = T.parse(line)
        if flags & (T.META | T.BAD):
            continue
        chrom = line.split(b"\t")[0]
        if chrom not in contigs:
            contigs.append(chrom)
        top = max(top, e)
        for edge in (b, max(e, b + 1)):
            for x in (edge - 1, edge, edge + 1):
                if x >= 0:
                    out.append((chrom, x, x + 1))
                    out.append((chrom, max(x - 20000, 0), x))
    out = sorted(set(out))
    rng = random.Random(seed)
    for _ in range(n_random if contigs else 0):
        beg = rng.randrange(0, top + 20000)
        out.append((rng.choice(contigs + [b"nowhere"]), beg, beg + rng.choice((1, 100, 20000, 1 << 22, 1 << 28))))
    return out


def check_queries_vcf(csi, vcf_gz):
    m = T.Members(vcf_gz)
    text = m.text()
    rows = T.data_rows(text)
    n = 0
    for contig, beg, end in regions_vcf(text):
        assert query_vcf(csi, m, contig, beg, end) == T.scan(rows, contig, beg, end), (contig, beg, end)
        n += 1
    return n


# ------------------------------------------------------------------------------------------ the new BAM inputs
class Case:
    """records under a header whose references have the lengths `ref_lens`; refuse: None, or (record number, kind) for the index"""

    def __init__(self, records, ref_lens, refuse=None):
        self.records, self.n_ref, self.refuse = list(records), len(ref_lens), refuse
        self.header = B.header(B.HEADERS["so_coordinate"], [("chr%d" % (i + 1), n) for i, n in enumerate(ref_lens)])


def _m(n):
    """a CIGAR of n reference bases (an operation holds 28 bits)"""
    ops = []
    while n > 0:
        ops.append((B.M, min(n, (1 << 28) - 1)))
        n -= ops[-1][1]
    return ops


D5, D6 = 1 << 29, 1 << 30          # reference lengths that give depth 5 and depth 6


def _cases():
    c = {}
    c["pos_2_29_minus_1"] = Case([B.rec("edge", 0, D5 - 1, 0, _m(2)), B.rec("front", 0, 7, 0, _m(5))], [D6])
    c["far"] = Case([B.rec("at_2_29", 0, 1 << 29, 0, _m(100)), B.rec("near_2_31", 0, (1 << 31) - 300, 16, _m(200)),
                     B.rec("to_2_32_minus_2", 0, (1 << 31) - 300, 0, _m((1 << 32) - 2 - ((1 << 31) - 300))), B.rec("low", 0, 3, 0, _m(50)),
                     B.rec("other", 1, (1 << 30) + 5, 0, _m(70))], [(1 << 31) - 1, D6])
    c["end_at_depth5_limit"] = Case([B.rec("last", 0, D5 - 10, 0, _m(10)), B.rec("first", 0, 5, 0, _m(10))], [D5])
    c["bin0_depth6"] = Case([B.rec("root", 0, D5 - 5, 0, _m(10)), B.rec("a", 0, 100, 0, _m(10)), B.rec("b", 0, D5 + 100, 0, _m(10))], [D6])
    leaf = []
    for k in (1, 2, 3, 8, 9, 64, 65, 4096):
        edge = k << 14
        leaf += [B.rec("l%d_m1" % k, 0, edge - 1, 0, _m(1)), B.rec("l%d_0" % k, 0, edge, 0, _m(1)), B.rec("l%d_p1" % k, 0, edge + 1, 0, _m(1)),
                 B.rec("l%d_x" % k, 0, edge - 1, 16, _m(2)), B.rec("l%d_to" % k, 0, edge - 20, 0, _m(20)), B.rec("l%d_over" % k, 0, edge - 20, 0, _m(21))]
    c["leaf_edges_depth5"] = Case(leaf, [D5])
    c["leaf_edges_depth6"] = Case(leaf, [D5 + 1])
    rnd = random.Random(41)
    c["running_maximum"] = Case([B.rec("long", 0, 100, 0, [(B.M, 10), (B.N, 5000000), (B.M, 10)])]
                                + [B.rec("s%d" % i, 0, rnd.randrange(200, 6000000), 0, _m(rnd.randrange(1, 300))) for i in range(300)]
                                + [B.rec("long2", 1, 1 << 20, 0, [(B.M, 5), (B.N, 1 << 24)])]
                                + [B.rec("t%d" % i, 1, (1 << 20) + rnd.randrange(1, 1 << 25), 16, _m(40)) for i in range(100)], [D5, D5])
    c["empty_references_between"] = Case([B.rec("r%d" % i, (0, 2, 4)[i % 3], 1000 * i, 0, _m(30)) for i in range(30)], [D5] * 6)
    c["unmapped_with_tid"] = Case([B.rec("u%d" % i, i % 2, 500 + 40000 * i, 4 if i % 3 == 0 else 0, _m(20) if i % 3 else ()) for i in range(40)]
                                  + [B.rec("n%d" % i, -1, -1, 4) for i in range(5)], [D5, D5])
    c["only_no_coordinate"] = Case([B.rec("n%d" % i, -1, -1, 4) for i in range(70)], [D5, D5])
    c["header_only"] = Case([], [D5, D6])
    c["long_record_depth5"] = Case([B.rec("long", 1, 300, 0, _m(10), size=70000)] + [B.rec("s%d" % i, 0, 900 - i, 0, _m(10)) for i in range(40)]
                                   + [B.rec("e%d" % i, 1, 400 + i, 0, _m(10)) for i in range(40)], [D5, D5])
    c["beyond_depth5"] = Case([B.rec("ok", 0, 5, 0, _m(10)), B.rec("beyond", 0, D5 - 10, 0, _m(11)), B.rec("ok2", 0, 50, 0, _m(10))], [1000],
                              refuse=(2, B.KIND_BEYOND))
    c["saturated_end"] = Case([B.rec("ok", 0, 5, 0, _m(10)), B.rec("ok2", 1, 50, 0, _m(10)),
                               B.rec("saturated", 0, (1 << 31) - 1, 0, _m((1 << 31) + 5))], [D6, D6], refuse=(3, B.KIND_BEYOND))
    return c


CASES = _cases()
INDEXABLE = sorted(name for name, case in CASES.items() if case.refuse is None)
REFUSED = sorted(name for name, case in CASES.items() if case.refuse is not None)


def all_indexable():
    """(label, case): every indexable input of tests/baicases.py and every new one"""
    return [("bai:" + name, B.CASES[name]) for name in B.INDEXABLE] + [("csi:" + name, CASES[name]) for name in INDEXABLE]

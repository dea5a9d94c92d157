"""The cases of the CRAM tests: record sets with the layout each is written in (cramwriter.Layout), and the rANS 4x8 corpus.
Everything is made once per process and not changed afterwards."""
import functools
import os
import random
import struct
import sys
from collections import Counter

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cramwriter as cw  # noqa: E402
from bamwriter import encode_record, parse_cigar, ref_len  # noqa: E402

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
FIXTURE_BAM = os.path.join(DATA, "NA12878.target_loci.sorted.bam")

REFS = [("chr1", 100000), ("chr2", 5000)]
HEADER = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
          + "@RG\tID:rg1\tSM:s1\tLB:lib1\n@RG\tID:rg2\tSM:s1\tLB:lib2\n")


def rec(name, flag, tid, pos, cigar, mtid=-1, mpos=-1, tlen=0, mapq=60, tags=()):
    return encode_record(dict(name=name, flag=flag, tid=tid, pos=pos, mapq=mapq, cigar=cigar, mtid=mtid, mpos=mpos, tlen=tlen, tags=list(tags)))[0][4:]


def chain(name, members, tags=()):
    """records of one template whose mate fields and template lengths are what the format's text gives an attached chain:
    members = [(flag without 0x20 / 0x8, tid, pos, cigar)]; a record's mate is the next one, the last one's the first"""
    ends = [pos + max(1, ref_len(parse_cigar(c))) if c != "*" else pos + 1 for _f, _t, pos, c in members]
    mapped = all(not f & 4 and t >= 0 and t == members[0][1] for f, t, _p, _c in members)
    lo = min(m[2] for m in members)
    hi = max(ends)
    first = next(k for k, m in enumerate(members) if m[2] == lo)
    out = []
    for k, (flag, tid, pos, cigar) in enumerate(members):
        mf, mt, mp, _mc = members[(k + 1) % len(members)]
        flag |= (0x20 if mf & 0x10 else 0) | (0x8 if mf & 0x4 else 0)
        tlen = 0 if not mapped else hi - lo if k == first else -(hi - lo)
        out.append((tid, pos, rec(name, flag, tid, pos, cigar, mt, mp, tlen, mapq=0 if flag & 4 else 37, tags=tags)))
    return out


def sort_records(items):
    """(tid, pos, record) in coordinate order, the unplaced last; stable"""
    return [r for _t, _p, r in sorted(items, key=lambda x: (x[0] if x[0] >= 0 else 1 << 30, x[1]))]


RG1 = [("RG", "Z", "rg1")]
EVERY_TAG = [("RG", "Z", "rg2"), ("XA", "A", "q"), ("Xc", "c", -5), ("XC", "C", 200), ("Xs", "s", -3000), ("XS", "S", 60000), ("Xi", "i", -70000),
             ("XI", "I", 4000000000), ("Xf", "f", 1.5), ("XZ", "Z", "some text"), ("XH", "H", "1AE301"), ("SA", "Z", "chr2,100,+,20M30S,60,0;"),
             ("Bc", "B", ("c", [-1, 2])), ("BC", "B", ("C", [1, 255])), ("Bs", "B", ("s", [-300, 9])), ("BS", "B", ("S", [65535])),
             ("Bi", "B", ("i", [-100000, 9, 9])), ("BI", "B", ("I", [4000000000])), ("Bf", "B", ("f", [0.5, -2.0])), ("Be", "B", ("c", []))]


@functools.lru_cache(maxsize=None)
def mixed_records():
    """one small file with every edge the record decoder has"""
    items = []
    items += chain("pairA", [(0x1 | 0x2 | 0x40, 0, 100, "50M"), (0x1 | 0x2 | 0x80 | 0x10, 0, 300, "50M")], RG1)
    items += chain("equal", [(0x1 | 0x40, 0, 500, "30M"), (0x1 | 0x80 | 0x10, 0, 500, "20M10S")], RG1)          # mates at equal starts
    items += chain("three", [(0x1 | 0x40, 0, 700, "40M10S"), (0x1 | 0x80 | 0x10, 0, 900, "50M"), (0x1 | 0x40 | 0x800, 0, 1500, "40H10M")], RG1)
    items.append((0, 1000, rec("everyop", 0, 0, 1000, "5H3S10M2I4M3D5M100N6M1P2M1I7M4S", tags=RG1)))
    items.append((0, 1100, rec("gap", 0x10, 0, 1100, "5S20M", tags=[("NM", "C", 0)])))                            # ends in a feature-free run
    items.append((0, 1200, rec("alltags", 0, 0, 1200, "25M", tags=EVERY_TAG)))
    items.append((0, 1300, rec("notags", 0x400, 0, 1300, "10M1D10M")))
    items.append((0, 99999, rec("lastbase", 0, 0, 99999, "1M", tags=RG1)))                                        # the contig's last base
    items += chain("far", [(0x1 | 0x40, 0, 2000, "50M"), (0x1 | 0x80, 1, 100, "50M")], RG1)                        # two references
    items += chain("halfmapped", [(0x1 | 0x40, 1, 200, "50M"), (0x1 | 0x80 | 0x4, 1, 200, "*")], RG1)
    # a detached record: its mate is not in the file
    items.append((1, 400, rec("lonely", 0x1 | 0x40 | 0x20, 1, 400, "50M", 1, 4000, 3650, tags=RG1)))
    for k in range(12):
        items += chain("p%02d" % k, [(0x1 | 0x2 | 0x40, 1, 1000 + 37 * k, "10S40M"), (0x1 | 0x2 | 0x80 | 0x10, 1, 1200 + 41 * k, "35M1I14M")], RG1)
    items += chain("unmappedpair", [(0x1 | 0x4 | 0x40, -1, -1, "*"), (0x1 | 0x4 | 0x80, -1, -1, "*")])           # AP 0
    return sort_records(items)


@functools.lru_cache(maxsize=None)
def many_groups():
    """300 read groups"""
    header = ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
              + "".join("@RG\tID:g%03d\tSM:s\tLB:l%d\n" % (k, k % 7) for k in range(300)))
    records = [rec("r%03d" % k, 0, 0, 10 * k, "20M", tags=[("RG", "Z", "g%03d" % ((k * 7) % 300))]) for k in range(300)]
    return header, records


def _core(kind):
    return lambda name: (kind,) if kind != "subexp" else ("subexp", 2)


def layouts():
    """(name, Layout) for the mixed records: every encoding where it is legal, every block method, every way of holding names,
    mates and positions"""
    L = cw.Layout
    stop_arrays = lambda name: ("stop", 0, cw._CID[name])                       # noqa: E731
    core_arrays = lambda name: ("len", ("beta",), ("huffman",))                  # noqa: E731
    z_stop = lambda tag: ("stop", 9, 70) if tag[2] in "ZH" else ("len", ("huffman",), ("external", 61))   # noqa: E731
    return [
        ("default", cw.default_layout(records_per_slice=20)),
        ("raw_external", L(records_per_slice=7)),
        ("huffman_core", L(ints=_core("huffman"), bytes_=_core("huffman"), records_per_slice=11)),
        ("beta_core", L(ints=_core("beta"), bytes_=_core("beta"), arrays=core_arrays, tags=lambda t: ("len", ("gamma",), ("beta",)))),
        ("gamma_core", L(ints=_core("gamma"), bytes_=_core("gamma"))),
        ("subexp_core", L(ints=_core("subexp"), bytes_=_core("subexp"), arrays=lambda n: ("len", ("subexp", 1), ("external", 5)))),
        ("stop_arrays", L(arrays=stop_arrays, tags=z_stop, names=True)),
        ("one_shared_block", L(ints=lambda n: ("external", 7), bytes_=lambda n: ("external", 7), arrays=lambda n: ("len", ("external", 7), ("external", 7)),
                               tags=lambda t: ("len", ("external", 7), ("external", 7)), method=cw.RANS1)),
        ("gzip", L(method=cw.GZIP, core_method=cw.GZIP, records_per_slice=9)),
        ("bzip2", L(method=cw.BZIP2, records_per_slice=13)),
        ("lzma", L(method=cw.LZMA, core_method=cw.LZMA)),
        ("rans1_everywhere", L(method=cw.RANS1, core_method=cw.RANS0, records_per_slice=16)),
        ("no_names", cw.default_layout(names=False, records_per_slice=20)),
        ("detached", L(attached=False, method=cw.RANS0)),
        ("no_names_detached", L(attached=False, names=False)),
        ("ap_absolute", L(ap_delta=False, method=cw.RANS0)),
        ("one_record_slices", cw.default_layout(records_per_slice=1)),
        ("split_pairs", L(records_per_slice=3, slices_per_container=4)),         # pairs cut by slice borders: detached
        ("multi_ref", L(multi_ref=True, records_per_slice=15, slices_per_container=2, method=cw.RANS0)),
        ("multi_ref_absolute", L(multi_ref=True, ap_delta=False, records_per_slice=100)),
        ("embedded_ref_flag", L(embedded_ref_flag=True)),
        ("feature_mix", L(feature_mix=True, method=cw.RANS0)),                   # X, B, b, i, q, Q: neighbours that merge
        ("feature_mix_core", L(feature_mix=True, ints=_core("huffman"), bytes_=_core("huffman"), arrays=core_arrays)),
        ("qual_arrays", L(qual_array=True, no_seq_unmapped=True, method=cw.RANS1)),
    ]


DAMAGED = [          # (knob, what the CramError says)
    ("crc", "CRC32 mismatch"),
    ("truncated", "truncated container"),
    ("freq", "does not sum to 4096"),
    ("method5", "samtools view -O cram,version=3.0"),
    ("major2", "major version 2"),
    ("golomb", "GOLOMB"),
    ("past_block", "reads past its block"),
]


# ------------------------------------------------------------------------------------------ the rANS corpus
def _skewed(rng, n, symbols):
    return bytes(rng.choice(symbols) for _ in range(n))


@functools.lru_cache(maxsize=None)
def rans_corpus():
    """[(name, block, output size, the bytes it decodes to or None, the status or None)]: None where only the host and the
    device have to agree"""
    rng = random.Random(20240229)
    plain = []
    for n in (0, 1, 3, 4, 5, 4099):
        plain.append(("size%d" % n, _skewed(rng, n, b"ACGTTTTTNNAA")))
    plain.append(("one_symbol", b"Q" * 1000))
    plain.append(("all_symbols", bytes(rng.sample(range(256), 256)) * 9 + bytes(range(256))))
    plain.append(("context_once", b"ab" * 700 + b"z" + b"ba" * 701))
    plain.append(("text", (b"chr1,1000,+,50M50S,60,0;" * 300)[:6001]))
    plain.append(("runs", b"".join(bytes([k]) * (k % 17 + 1) for k in range(256))))
    out = []
    for name, data in plain:
        for order in (0, 1):
            out.append(("%s_o%d" % (name, order), cw.rans_encode(data, order), len(data), data, 0))
    good0, good1 = cw.rans_encode(plain[5][1], 0), cw.rans_encode(plain[5][1], 1)
    n = len(plain[5][1])

    def resized(block, payload):
        return block[:1] + struct.pack("<I", len(payload)) + block[5:9] + payload
    out.append(("bad_sum_o0", cw.rans_encode(plain[5][1], 0, bad_sum=True), n, None, 2))
    out.append(("bad_sum_o1", cw.rans_encode(plain[5][1], 1, bad_sum=True), n, None, 2))
    out.append(("input_runs_out_o0", resized(good0, good0[9:-40]), n, None, 3))
    out.append(("input_runs_out_o1", resized(good1, good1[9:-40]), n, None, 3))
    out.append(("table_runs_out", resized(good0, good0[9:12]), n, None, 2))
    table = len(cw._table(cw._normalise(Counter(plain[5][1]))))
    out.append(("no_states", resized(good0, good0[9:9 + table + 7]), n, None, 3))
    out.append(("order_byte_2", b"\x02" + good0[1:], n, None, 1))
    out.append(("size_field_wrong", good0[:1] + struct.pack("<I", len(good0)) + good0[5:], n, None, 1))
    out.append(("output_size_wrong", good0, n + 1, None, 1))
    out.append(("shorter_than_header", good0[:5], 7, None, 1))
    out.append(("empty_block", b"", 3, None, 1))
    out.append(("order1_nothing", b"\x01" + struct.pack("<II", 0, 0), 0, None, 5))
    for k in range(6):
        junk = bytes(rng.randrange(256) for _ in range(200 + 31 * k))
        out.append(("junk%d" % k, bytes([k & 1]) + struct.pack("<II", len(junk), 500) + junk, 500, None, None))
    for k, block in enumerate((good0, good1)):          # a damaged state or byte: whatever it decodes to, both sides say the same
        hurt = bytearray(block)
        for at in range(len(hurt) - 30, len(hurt) - 20):
            hurt[at] ^= 0x5A
        out.append(("hurt_bytes_o%d" % k, bytes(hurt), n, None, None))
    return out

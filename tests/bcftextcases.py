"""Hand-built BCF2.2 streams for the decoder (svtyper_amd/csrc/svt_bcf_text.h), made with struct from the published format: a file
whose header carries permuted and sparse IDX= as bcftools writes them, with the text its records are to print as; a float vector
that walks the edges of the exact %g rule; and one stream per refusal kind -- a good record, the bad one, a good one, so that the
refused record is number 2.  Nothing here imports svtyper_amd."""
import struct

import numpy as np

MISSING = {1: -128, 2: -32768, 3: -2147483648}
EOV = {1: -127, 2: -32767, 3: -2147483647}
FLOAT_MISSING, FLOAT_EOV = 0x7F800001, 0x7F800002
_FMT = {1: "b", 2: "h", 3: "i"}


def _kind(values):
    if all(-120 <= v <= 127 for v in values):
        return 1
    return 2 if all(-32760 <= v <= 32767 for v in values) else 3


def desc(count, kind):
    if count < 15:
        return bytes([count << 4 | kind])
    return bytes([0xF0 | kind]) + ints([count])


def ints(values, kind=None):
    kind = kind or _kind(values)
    return desc(len(values), kind) + struct.pack("<%d%s" % (len(values), _FMT[kind]), *values)


def floats(bits):
    return desc(len(bits), 5) + struct.pack("<%dI" % len(bits), *bits)


def chars(b):
    return desc(len(b), 7) + b


def per_sample(kind, count, rows):
    """a FORMAT block: one descriptor, then every sample's `count` values (bytes for kind 7, uint32 bits for 5, ints else)"""
    out = desc(count, kind)
    for row in rows:
        out += row if kind == 7 else struct.pack("<%d%s" % (count, "I" if kind == 5 else _FMT[kind]), *row)
    return out


def f32(x):
    return int(np.float32(x).view(np.uint32))


def record(chrom, pos0, rlen, qual, ident, alleles, filt, info, fmt, n_sample, n_info=None, n_fmt=None, n_allele=None):
    """`qual`: float32 bits; `filt`: the typed vector's bytes; `info` / `fmt`: [(key index, the typed value's / block's bytes)]"""
    shared = struct.pack("<iiiIII", chrom, pos0, rlen, qual, (len(alleles) if n_allele is None else n_allele) << 16 | (len(info) if n_info is None else n_info),
                         (len(fmt) if n_fmt is None else n_fmt) << 24 | n_sample)
    shared += chars(ident) + b"".join(chars(a) for a in alleles) + filt + b"".join(ints([k]) + v for k, v in info)
    indiv = b"".join(ints([k]) + v for k, v in fmt)
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


def stream(header, records):
    text = header.encode() + b"\0"
    return b"BCF\2\2" + struct.pack("<I", len(text)) + text + b"".join(records)


# ------------------------------------------------------------------------------------------ IDX=: permuted and sparse
IDX_HEADER = "".join(l + "\n" for l in (
    "##fileformat=VCFv4.2",
    '##FILTER=<ID=PASS,Description="All filters passed",IDX=0>',
    '##FILTER=<ID=q10,Description="Quality below 10,IDX=9 stays inside quotes",IDX=7>',
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth",IDX=3>',
    '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency",IDX=1>',
    '##INFO=<ID=DB,Number=0,Type=Flag,Description="In the database",IDX=12>',
    '##INFO=<ID=NOTE,Number=1,Type=String,Description="A note",IDX=4>',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype",IDX=5>',
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Depth",IDX=3>',
    '##FORMAT=<ID=FT,Number=1,Type=String,Description="Sample filter",IDX=8>',
    "##contig=<ID=chrB,length=1000,IDX=2>",
    "##contig=<ID=chrA,length=2000,IDX=0>",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2"))
IDX_PRINTED = IDX_HEADER.replace(",IDX=0>", ">").replace(",IDX=7>", ">").replace(",IDX=3>", ">").replace(",IDX=1>", ">").replace(",IDX=12>", ">") \
    .replace(",IDX=4>", ">").replace(",IDX=5>", ">").replace(",IDX=8>", ">").replace(",IDX=2>", ">")
assert IDX_PRINTED.count("IDX=") == 1               # (the one inside quotes)


def good_record(chrom=2, n_sample=2):
    return record(chrom, 99, 1, f32(12.5), b"rs1", [b"A", b"T"], ints([0]), [(3, ints([14])), (12, b"\x00")],
                  [(5, per_sample(1, 2, [[2, 4], [2, 5]][:n_sample])), (3, per_sample(1, 1, [[7], [MISSING[1]]][:n_sample]))], n_sample)


GOOD_LINE = "chrB\t100\trs1\tA\tT\t12.5\tPASS\tDP=14;DB\tGT:DP\t0/1:7\t0|1:."


def idx_stream():
    """-> (stream, the text it is to print)"""
    records = [
        good_record(),
        record(0, 0, 3, FLOAT_MISSING, b"", [b"ACG", b"A", b"<DEL>"], ints([7, 0]), [(1, floats([f32(0.25), FLOAT_MISSING, f32(1e-3)])), (4, chars(b"a b")),
                                                                                 (3, ints([MISSING[2], 300], 2))],
               [(5, per_sample(2, 3, [[2, 4, EOV[2]], [0, 2, 7]])), (8, per_sample(7, 4, [b"PASS", b"q\0\0\0"])), (3, per_sample(3, 1, [[70000], [EOV[3]]]))], 2),
        record(2, 499, 1, f32(0.0), b"x", [b"N"], desc(0, 0), [], [], 2),
        record(0, 9, 1, f32(-3.5), b"y", [b"N", b"<DUP>"], desc(0, 1), [(1, floats([FLOAT_EOV]))], [(5, per_sample(1, 1, [[EOV[1]], [0]]))], 2),
    ]
    lines = [GOOD_LINE,
             "chrA\t1\t.\tACG\tA,<DEL>\t.\tq10;PASS\tAF=0.25,.,0.001;NOTE=a b;DP=.,300\tGT:FT:DP\t0/1:PASS:70000\t./0|2:q:.",
             "chrB\t500\tx\tN\t.\t0\t.\t.",
             "chrA\t10\ty\tN\t<DUP>\t-3.5\t.\tAF=.\tGT\t.\t."]
    return stream(IDX_HEADER, records), IDX_PRINTED + "".join(l + "\n" for l in lines)


# ------------------------------------------------------------------------------------------ floats at the edges of the %g rule
def edge_floats():
    """float32 bit patterns: the envelope's ends and both neighbours, every decade's ends, ties at six digits (the float32 grid is
    fine enough for exact halves below 2^17), values that round up into the next decade, seeded values across the envelope and
    outside it, the non-finite ones"""
    vals = [0.0, -0.0, 1e-4, 1e6, 999999.0, 999999.5, 999999.4375, 999999.9375, 1000000.0, 100000.5, 100001.5, 100002.5, -100000.5, 131071.5, 65536.5,
            0.5, 0.25, 0.125, 1.0, 10.0, 100.0, 12345.6, 123456.0, 1234565.0, 0.000123456, 0.00099999997, 0.001, 0.0099999998, 0.01, 0.099999994, 0.1, 0.9999995,
            0.99999994, 9.999995, 9.9999995, 99.99995, 99999.95, 99999.99, 1e-5, 4.7e-7, 1e7, 1e22, 3.4028235e38, 1e-38, 1e-45, 2.675, 1.005, 285.53, 0.48,
            float("inf"), float("-inf")]
    bits = [f32(v) for v in vals]
    for b in list(bits):                            # both float32 neighbours of every value
        if b & 0x7FFFFFFF not in (0, 0x7F800000):
            bits += [b + 1, b - 1]
    rnd = np.random.RandomState(20250101)
    bits += [f32(v) for v in 10.0 ** rnd.uniform(-5, 7, 1500) * rnd.choice((-1, 1), 1500)]
    bits += [f32(round(float(v), 2)) for v in rnd.uniform(0, 3000, 500)]
    bits += [0x7FC00000, 0xFFC00000, 0x7F800003, 0x00000001, 0x807FFFFF, 0x00800000]        # nans of both signs, subnormals, the least normal
    return [b for b in bits if b not in (FLOAT_MISSING, FLOAT_EOV)]


FLOAT_HEADER = "".join(l + "\n" for l in ("##fileformat=VCFv4.2", '##INFO=<ID=V,Number=.,Type=Float,Description="Values">', "##contig=<ID=c>",
                                          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"))


def float_stream(bits):
    """one record per float: INFO V=<the float>, QUAL the same float"""
    return stream(FLOAT_HEADER, [record(0, k, 1, b, b"", [b"N"], desc(0, 0), [(1, floats([b]))], [], 0) for k, b in enumerate(bits)])


# ------------------------------------------------------------------------------------------ refusals
def _patched(rec, shared_edit=None, indiv_edit=None):
    """`rec` with its shared / individual part passed through an edit, the two lengths set again"""
    ls, li = struct.unpack_from("<II", rec)
    shared, indiv = rec[8:8 + ls], rec[8 + ls:8 + ls + li]
    shared = shared_edit(shared) if shared_edit else shared
    indiv = indiv_edit(indiv) if indiv_edit else indiv
    return struct.pack("<II", len(shared), len(indiv)) + shared + indiv


def _sub(at, new, old_len=None):
    return lambda part: part[:at] + new + part[at + (len(new) if old_len is None else old_len):]


def refusals():
    """[(name, kind as native_reads.BCF_TEXT_KINDS says it, the bad record's bytes)] against IDX_HEADER"""
    good = good_record()
    ls = struct.unpack_from("<I", good)[0]
    id_at = 24                                      # the ID's descriptor in the shared part: 0x37 'r' 's' '1'
    filt_at = id_at + 4 + 2 + 2                     # ... 0x17 'A' 0x17 'T', then FILTER: 0x11 0x00
    info_at = filt_at + 2                           # 0x11 0x03 0x11 0x0e | 0x11 0x0c 0x00
    out = [
        ("l_shared_below_24", "truncated", struct.pack("<II", 20, 0) + good[8:28]),
        ("contig_beyond", "index", good_record(chrom=5)),
        ("contig_in_a_hole", "index", good_record(chrom=1)),
        ("contig_negative", "index", good_record(chrom=-1)),
        ("filter_is_an_info_key", "index", _patched(good, _sub(filt_at + 1, b"\x03"))),
        ("filter_missing_value", "index", _patched(good, _sub(filt_at + 1, b"\x80"))),
        ("info_key_is_format_only", "index", _patched(good, _sub(info_at + 1, b"\x05"))),
        ("info_key_beyond", "index", _patched(good, _sub(info_at + 1, b"\x63"))),
        ("info_key_in_a_hole", "index", _patched(good, _sub(info_at + 1, b"\x02"))),
        ("format_key_is_info_only", "index", _patched(good, None, _sub(1, b"\x01"))),
        ("n_sample_three", "samples", _patched(good, _sub(20, struct.pack("<I", 2 << 24 | 3)))),
        ("n_sample_none", "samples", _patched(good, _sub(20, struct.pack("<I", 2 << 24 | 0)))),
        ("type_four", "type", _patched(good, _sub(info_at + 2, b"\x14"))),
        ("type_six_in_format", "type", _patched(good, None, _sub(2, b"\x26"))),
        ("type_eight", "type", _patched(good, _sub(id_at, b"\x38"))),
        ("id_as_integers", "type", _patched(good, _sub(id_at, b"\x31"))),
        ("key_as_characters", "type", _patched(good, _sub(info_at, b"\x17"))),
        ("key_of_two_integers", "type", _patched(good, _sub(info_at, b"\x21\x03\x03", 2))),
        ("long_count_as_float", "count", _patched(good, _sub(id_at, b"\xf7\x15\x00\x00\x40\x40", 1))),
        ("long_count_of_two", "count", _patched(good, _sub(id_at, b"\xf7\x21\x03\x03", 1))),
        ("long_count_negative", "count", _patched(good, _sub(id_at, b"\xf7\x11\xf0", 1))),
        ("long_count_beyond_the_part", "count", _patched(good, _sub(id_at, b"\xf7\x12\x00\x40", 1))),
        ("vector_beyond_the_part", "count", _patched(good, _sub(info_at + 2, b"\xe3"))),
        ("format_block_beyond_the_part", "count", _patched(good, None, _sub(2, b"\x42"))),
        ("gt_as_characters", "gt", _patched(good, None, _sub(2, b"\x27"))),
        ("gt_as_floats", "gt", _patched(good, None, lambda p: p[:2] + b"\x15" + p[3:7] + b"\0\0\0\0" + p[7:])),
        ("shared_part_with_a_tail", "length", _patched(good, lambda p: p + b"\x00")),
        ("individual_part_with_a_tail", "length", _patched(good, None, lambda p: p + b"\x11")),
        ("fewer_info_than_n_info", "length", _patched(good, _sub(16, struct.pack("<I", 2 << 16 | 3)))),
        ("more_info_than_n_info", "length", _patched(good, _sub(16, struct.pack("<I", 2 << 16 | 1)))),
        ("fewer_keys_than_n_fmt", "length", _patched(good, _sub(20, struct.pack("<I", 3 << 24 | 2)))),
    ]
    assert ls == info_at + 7
    return out


def refusal_stream(bad):
    return stream(IDX_HEADER, [good_record(), bad, good_record()])

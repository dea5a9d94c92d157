"""The corpus the BCF encoder is held to: a header that declares every Type x Number kind, data lines that walk the record rule's
edges, seeded random lines, the refusals, and texts of chosen shapes for the device tests.  Nothing here imports svtyper_amd; the
yardstick that reads the encoder's output back is tests/bcfreader.py.

`in_envelope` restates, from the issue's wording and not from the encoder, which float tokens the device computes itself: a plain
decimal (sign, digits, a point, an exponent), at most 15 digits from the first nonzero one to the last one written, and a decimal
exponent of magnitude at most 22 once the fraction digits are folded in.  Hex floats are left out of the corpus: Python's
float() does not read them, so the yardstick has no value for them."""
import random
import re

SAMPLES = ("S1", "S2", "S3")

HEADER_LINES = (
    "##fileformat=VCFv4.2",
    "##fileDate=20240101",
    "##reference=grch37",
    '##FILTER=<ID=LowQual,Description="Low quality">',
    '##FILTER=<ID=q10,Description="Quality below 10">',
    '##INFO=<ID=SVTYPE,Number=1,Type=String,Description="Type of structural variant">',
    '##INFO=<ID=SVLEN,Number=.,Type=Integer,Description="Difference in length between REF and ALT alleles">',
    '##INFO=<ID=END,Number=1,Type=Integer,Description="End position, with a comma, inside quotes">',
    '##INFO=<ID=CIPOS,Number=2,Type=Integer,Description="Confidence interval around POS">',
    '##INFO=<ID=IMPRECISE,Number=0,Type=Flag,Description="Imprecise structural variation">',
    '##INFO=<ID=SECONDARY,Number=0,Type=Flag,Description="Secondary breakend">',
    '##INFO=<ID=MATEID,Number=.,Type=String,Description="ID of mate breakends">',
    '##INFO=<ID=EVENT,Number=1,Type=String,Description="ID of event">',
    '##INFO=<ID=SUP,Number=1,Type=Integer,Description="Supporting pieces of evidence">',
    '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele frequency">',
    '##INFO=<ID=SCORE,Number=1,Type=Float,Description="A score">',
    '##INFO=<ID=PRPOS,Number=.,Type=Float,Description="Breakpoint probability dist">',
    '##INFO=<ID=BIG,Number=.,Type=Integer,Description="Integers of every width">',
    '##INFO=<ID=CH,Number=1,Type=Character,Description="One character">',
    '##INFO=<ID=STRANDS,Number=R,Type=String,Description="Strand orientation">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##FORMAT=<ID=SUP,Number=1,Type=Integer,Description="Supporting pieces of evidence, per sample">',
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">',
    '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled likelihoods">',
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Allele depths">',
    '##FORMAT=<ID=GL,Number=G,Type=Float,Description="Genotype likelihoods">',
    '##FORMAT=<ID=AB,Number=1,Type=Float,Description="Allele balance">',
    '##FORMAT=<ID=FT,Number=1,Type=String,Description="Sample filter">',
    '##FORMAT=<ID=TAG,Number=.,Type=String,Description="Free tags">',
    '##FORMAT=<ID=C,Number=1,Type=Character,Description="One character per sample">',
    "##contig=<ID=chr1,length=248956422>",
    "##contig=<ID=chr2,length=242193529>",
    "##contig=<ID=chrX,length=156040895,assembly=b37>",
    '##ALT=<ID=DEL,Description="Deletion">',
)
# what the encoder must derive from them (order of first appearance, PASS first, SUP once)
STRINGS = ["PASS", "LowQual", "q10", "SVTYPE", "SVLEN", "END", "CIPOS", "IMPRECISE", "SECONDARY", "MATEID", "EVENT", "SUP", "AF", "SCORE", "PRPOS", "BIG",
           "CH", "STRANDS", "GT", "GQ", "PL", "AD", "GL", "AB", "FT", "TAG", "C"]
CONTIGS = ["chr1", "chr2", "chrX"]
L_REF_MAX = 248956422


def header(samples=SAMPLES, fmt=True):
    cols = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO" + ("\tFORMAT\t" + "\t".join(samples) if samples and fmt else "")
    return "\n".join(HEADER_LINES) + "\n" + cols + "\n"


def in_envelope(token):
    m = re.fullmatch(r"[+-]?(\d*)(?:\.(\d*))?(?:[eE]([+-]?\d+))?", token)
    if not m or not (m.group(1) or m.group(2)):
        return False
    whole, frac, exp = m.group(1) or "", m.group(2) or "", int(m.group(3) or 0)
    digits = (whole + frac).lstrip("0")
    return len(digits) <= 15 and abs(exp - len(frac)) <= 22


FLOATS_IN = ["0", "-0", "0.00", "1.00", "0.25", "99.99", "-3.25", "+7", "5.", ".5", "1e-05", "4.7e-07", "1.2e+02", "9.9E3", "123456789012345",
             "0.123456789012345", "1e22", "1e-22", "1.5e23", "123456789012345e7", "0.000001", "33", "1000000", "0.1", "0.7", "2.675", "1.005"]
FLOATS_OUT = ["1234567890123456", "0.1234567890123456", "1e23", "1e-23", "2.3e-22", "nan", "inf", "-inf", "1e400", "1e-400", "3.4028235e38", "1e39",
              "Infinity", "12345678901234567890.5"]
assert all(in_envelope(t) for t in FLOATS_IN) and not any(in_envelope(t) for t in FLOATS_OUT)

INT_EDGES = [-121, -120, 127, 128, -32761, -32760, 32767, 32768, -2147483640, 2147483647, 0, -1]


def _line(chrom="chr1", pos=100, ident=".", ref="N", alt="<DEL>", qual=".", filt=".", info=".", fmt=None, samples=()):
    cols = [chrom, str(pos), ident, ref, alt, qual, filt, info]
    if fmt is not None:
        cols += [fmt] + list(samples)
    return "\t".join(cols)


def _fixed_lines():
    """[(name, line)]: three samples wherever there is a FORMAT column"""
    L = []
    add = lambda name, **kw: L.append((name, _line(**kw)))
    add("sites_only")
    add("pass_filter", filt="PASS", qual="12.50", info="SVTYPE=DEL;END=250;SVLEN=-150")
    add("named_filters", filt="LowQual;q10", info="SVTYPE=DEL;END=1000")
    add("flags_and_dots", info="IMPRECISE;SECONDARY;SVLEN=.;AF=.;EVENT=.;CIPOS=-10,.")
    add("bnd", ident="7_1", ref="A", alt="A]chr2:5000]", qual="0.00", info="SVTYPE=BND;MATEID=7_2;EVENT=7;STRANDS=+-:4")
    add("bnd_mate", chrom="chr2", pos=5000, ident="7_2", ref="N", alt="[chr1:100[N", info="SVTYPE=BND;MATEID=7_1,7_3;SECONDARY")
    add("two_alts", ref="ACGT", alt="A,ACGTT", info="AF=0.25,0.5;STRANDS=++,--,+-", qual="1e-05")
    add("alt_dot", ref="ACGT", alt=".", ident="rs1;rs2")
    add("end_before_pos", pos=5000, info="END=100")
    add("end_list", pos=10, info="END=40,50")
    add("pos_zero", pos=0, info="SVTYPE=INS")
    add("pos_one", pos=1, info="END=1")
    add("pos_top", chrom="chrX", pos=2147483646, info="SVTYPE=DEL")
    add("character", info="CH=x;SUP=12")
    add("long_string", info="EVENT=" + "e" * 300, ident="i" * 20, ref="A" * 15, alt="C" * 14 + ",<INS:ME:" + "L" * 40 + ">")
    add("many_ints", info="SVLEN=" + ",".join(str(i) for i in range(20)) + ";BIG=" + ",".join(["."] * 15))
    for v in INT_EDGES:
        add("info_int_%d" % v, info="BIG=%d" % v)
        add("info_int_pair_%d" % v, info="BIG=5,%d,." % v)
    for k, t in enumerate(FLOATS_IN + FLOATS_OUT):
        add("info_float_%d" % k, info="SCORE=%s;PRPOS=%s,.,1.5" % (t, t))
        add("qual_float_%d" % k, qual=t)
    gts = ["0/1", "1|0", "./.", ".", "1", "0/0", "1/1", ".|.", "0|1|2", "2/1", "0/.", "70/1"]
    for k in range(0, len(gts), 3):
        add("gt_%d" % k, fmt="GT", samples=gts[k:k + 3], alt="<DEL>,<DUP>" + ",<X>" * 70)
    add("gt_alone_dot", fmt="GT", samples=[".", ".", "."])
    add("gt_haploid_mix", fmt="GT:GQ", samples=["1:7", "0/1:8", ".:9"])
    add("unequal_vectors", fmt="GT:AD:PL:GL", samples=["0/1:3,4:0,10,200:-0.01,-1.5,-20", "0/0:5:.:.", "./.:.,.,7:1,2:-3"])
    add("unequal_strings", fmt="GT:FT:TAG:C", samples=["0/1:PASS:a,bc,def:x", "0/0:LowQual;q10:.:y", "1/1:.::z"])
    add("short_samples", fmt="GT:GQ:AB:FT:AD", samples=["0/1:5:0.5:PASS:1,2", "0/0", "./.:7:."])
    add("all_missing", fmt="GT:GQ:AB:PL", samples=["./.:.:.:.", "./.:.:.:.", "./.:.:.:."])
    for v in INT_EDGES:
        add("fmt_int_%d" % v, fmt="GT:SUP:AD", samples=["0/1:%d:1,2" % v, "0/0:3:%d,%d,." % (v, v), "1/1:.:0"])
    for k, t in enumerate(FLOATS_IN + FLOATS_OUT):
        add("fmt_float_%d" % k, fmt="GT:AB:GL", samples=["0/1:%s:-1,%s" % (t, t), "0/0:.:%s" % t, "1/1:0.5:.,.,%s" % t])
    add("sso_shape", chrom="chr1", pos=869423, ident="1", ref="N", alt="<DEL>", qual="285.53", filt=".",
        info="SVTYPE=DEL;SVLEN=-857;END=870280;STRANDS=+-:6;IMPRECISE;CIPOS=-1,34;SUP=6;AF=0.5",
        fmt="GT:GQ:SUP:AB:GL:PL:AD", samples=["0/1:200:21:0.48:-128,-10,-80:1285,100,800:25,21", "0/0:99:0:0:-0,-9,-90:0,90,900:30,0", "./.:.:.:.:.:.:."])
    return L


def _random_lines(seed=20240917, n=160):
    rnd = random.Random(seed)
    out = []
    floats = FLOATS_IN
    for i in range(n):
        chrom = rnd.choice(CONTIGS)
        pos = rnd.choice((1, 2, 16383, 16384, 16385, 1 << 20, rnd.randrange(1, 150000000)))
        info = []
        if rnd.random() < 0.8:
            info.append("SVTYPE=" + rnd.choice(("DEL", "DUP", "INV", "BND")))
        if rnd.random() < 0.6:
            info.append("END=%d" % (pos + rnd.choice((0, 1, 50, 16384, 1 << 17, 3000000))))
        if rnd.random() < 0.5:
            info.append("SVLEN=" + ",".join(str(rnd.choice(INT_EDGES + [rnd.randrange(-70000, 70000)])) for _ in range(rnd.randrange(1, 4))))
        if rnd.random() < 0.4:
            info.append("AF=" + ",".join(rnd.choice(floats + ["."]) for _ in range(rnd.randrange(1, 3))))
        if rnd.random() < 0.3:
            info.append(rnd.choice(("IMPRECISE", "SECONDARY")))
        if rnd.random() < 0.3:
            info.append("SUP=%d" % rnd.randrange(0, 500))
        rnd.shuffle(info)
        keys = ["GT"] + [k for k in ("GQ", "SUP", "AB", "GL", "PL", "AD", "FT", "TAG") if rnd.random() < 0.6]
        samples = []
        for _s in SAMPLES:
            parts = []
            for k in keys:
                if k == "GT":
                    parts.append(rnd.choice(("0/0", "0/1", "1/1", "./.", "1|0", ".")))
                elif k in ("GQ", "SUP"):
                    parts.append(rnd.choice((".", str(rnd.randrange(0, 300)), str(rnd.choice(INT_EDGES)))))
                elif k == "AB":
                    parts.append(rnd.choice(floats + ["."]))
                elif k == "GL":
                    parts.append(",".join("%.2f" % -rnd.uniform(0, 300) for _ in range(rnd.choice((1, 3)))))
                elif k in ("PL", "AD"):
                    parts.append(",".join(rnd.choice((".", str(rnd.randrange(0, 40000)))) for _ in range(rnd.randrange(1, 4))))
                elif k == "FT":
                    parts.append(rnd.choice(("PASS", "LowQual", ".", "q10;LowQual")))
                else:
                    parts.append(rnd.choice(("a", "bb,c", ".", "")))
            if rnd.random() < 0.1:
                parts = parts[:rnd.randrange(1, len(parts) + 1)]
            samples.append(":".join(parts))
        out.append(("random_%d" % i, _line(chrom, pos, rnd.choice((".", "v%d" % i)), rnd.choice(("N", "A", "ACGTACGT")), rnd.choice(("<DEL>", "T", "<DUP>,<INV>")),
                                           rnd.choice((".", "%.2f" % rnd.uniform(0, 3000), "%.2g" % rnd.uniform(0, 1e-4), "%.0f" % rnd.uniform(0, 1e6))),
                                           rnd.choice((".", "PASS", "LowQual", "q10;LowQual")), ";".join(info) or ".", ":".join(keys), samples)))
    return out


LINES = _fixed_lines() + _random_lines()


def line_in_envelope(line):
    """no float token of `line` lies outside the envelope (any column: a token that is no float is no float token)"""
    return not any(t in FLOATS_OUT for t in re.split(r"[\t;=:,]", line))


# (name, line, kind as native_reads.BCF_KINDS says it, the key or column the error names)
REFUSALS = [
    ("contig", _line(chrom="chr9"), "contig", "CHROM"),
    ("info_key", _line(info="SVTYPE=DEL;NOPE=1"), "info_key", "NOPE"),
    ("info_key_is_format_only", _line(info="GQ=1"), "info_key", "GQ"),
    ("format_key", _line(fmt="GT:XX", samples=["0/1:1"] * 3), "format_key", "XX"),
    ("format_key_is_info_only", _line(fmt="GT:END", samples=["0/1:1"] * 3), "format_key", "END"),
    ("filter", _line(filt="PASS;nope"), "filter", "nope"),
    ("filter_is_info_key", _line(filt="SVTYPE"), "filter", "SVTYPE"),
    ("int_text", _line(info="SUP=12x"), "info_value", "SUP"),
    ("int_empty", _line(info="SVLEN=1,,2"), "info_value", "SVLEN"),
    ("int_float", _line(info="SUP=1.5"), "info_value", "SUP"),
    ("int_below_floor", _line(info="BIG=-2147483641"), "info_value", "BIG"),
    ("int_above_top", _line(info="BIG=2147483648"), "info_value", "BIG"),
    ("int_eleven_digits", _line(info="BIG=12345678901"), "info_value", "BIG"),
    ("float_text", _line(info="SCORE=abc"), "info_value", "SCORE"),
    ("float_trailing", _line(info="SCORE=1.5x"), "info_value", "SCORE"),
    ("float_half_exponent", _line(info="SCORE=1e"), "info_value", "SCORE"),
    ("qual_text", _line(qual="high"), "qual", "QUAL"),
    ("fmt_int_text", _line(fmt="GT:GQ", samples=["0/1:1", "0/0:x", "1/1:2"]), "format_value", "GQ"),
    ("fmt_int_range", _line(fmt="GT:GQ", samples=["0/1:1", "0/0:2147483648", "1/1:2"]), "format_value", "GQ"),
    ("fmt_float_text", _line(fmt="GT:AB", samples=["0/1:1", "0/0:0.5", "1/1:zz"]), "format_value", "AB"),
    ("gt_text", _line(fmt="GT", samples=["0/1", "a/b", "1/1"]), "format_value", "GT"),
    ("gt_empty_allele", _line(fmt="GT", samples=["0/1", "0/", "1/1"]), "format_value", "GT"),
    ("too_many_fields", _line(fmt="GT:GQ", samples=["0/1:1", "0/0:2:3", "1/1:2"]), "format_value", "GQ"),
    ("pos_top", _line(pos=2147483647), "pos", "POS"),
    ("pos_beyond", _line(pos=4294967296), "pos", "POS"),
    ("pos_text", _line(pos="12a"), "pos", "POS"),
    ("pos_negative", _line(pos=-5), "pos", "POS"),
    ("seven_columns", "chr1\t100\t.\tN\t<DEL>\t.\t.", "columns", None),
    ("empty_line", "", "columns", None),
    ("format_without_samples", _line(fmt="GT"), "samples", "FORMAT"),
    ("two_samples", _line(fmt="GT", samples=["0/1", "0/0"]), "samples", "FORMAT"),
    ("four_samples", _line(fmt="GT", samples=["0/1"] * 4), "samples", "FORMAT"),
]


def corpus_text(names=None, envelope=None):
    """the header and the named LINES (all by default; envelope=True / False: those inside / with a token outside)"""
    body = [line for name, line in LINES if (names is None or name in names) and (envelope is None or line_in_envelope(line) == envelope)]
    return header() + "".join(l + "\n" for l in body)


def shaped_text(n_lines, n_samples, seed=5):
    """`n_lines` data lines of `n_samples` samples each, cycling through the shapes of the corpus that do not depend on the sample
    count: sites-only lines widened with a FORMAT column of seeded values"""
    rnd = random.Random(seed * 1000003 + n_lines * 131 + n_samples)
    samples = tuple("S%d" % i for i in range(n_samples))
    out = [header(samples)]
    for i in range(n_lines):
        cols = []
        for s in range(n_samples):
            gt = rnd.choice(("0/0", "0/1", "1/1", "./.", "."))
            cols.append("%s:%s:%d:%s:%s:%s" % (gt, rnd.choice((".", str(rnd.randrange(0, 201)))), rnd.choice(INT_EDGES + [rnd.randrange(0, 100)]),
                                               rnd.choice(FLOATS_IN), ",".join("%.2f" % -rnd.uniform(0, 200) for _ in range(rnd.choice((1, 3)))),
                                               rnd.choice(("PASS", ".", "LowQual;q10"))))
        out.append(_line(rnd.choice(CONTIGS), rnd.randrange(1, 1 << 27), "v%d" % i, "N", "<DEL>", "%.2f" % rnd.uniform(0, 999), rnd.choice((".", "PASS")),
                         "SVTYPE=DEL;END=%d;SUP=%d;AF=%s" % ((1 << 27) + i, rnd.randrange(0, 100000), rnd.choice(FLOATS_IN)), "GT:GQ:SUP:AB:GL:FT", cols) + "\n")
    return "".join(out)


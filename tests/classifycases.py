"""The corpus of svtyper_amd.classify: synthetic cohort VCFs with per-sample CN and AB (svtyper writes no CN, so nothing real
exists), shared by tests/test_classify_host.py, tests/test_classify_native.py, tests/test_classify_device.py and
tests/golden/make_golden_classify.py.  Everything is built in code and deterministic.

A case: name, vcf, gender, exclude (text or None), annotation (the BED's text or None), options (f_overlap, slope_threshold,
rsquared_threshold), and what the case was built for: slow_lines (the DEL/DUP lines outside the envelope of
svtyper_amd/csrc/svt_vcf_classify.h that the host's plain C++ decides), low ({0-based body line: the CN list the median is
taken of}, for the autosomal lines of the low-frequency test), error (None, or the 1-based line of the VCF that ends the
run) and kind (of an error: which SVT_CLASSIFY_BAD_* the native code names it by, as the name behind that prefix; None for an
error of the annotation, which is Python's).  What the reference's script gives for a case is in
tests/golden/classify_cases.json.gz, by name.

CN and AB carry two to four decimals, so that the regression's r2 and slope stay far from their thresholds (the generator of
the goldens asserts 1e-6) whatever order the sums are taken in.
"""
SAMPLE_COUNTS = (1, 9, 10, 63, 64, 65, 130, 255, 256, 257)
CAPACITY = 4096                                     # native_reads.CLASSIFY_CAPACITY
OPTIONS = dict(f_overlap=0.9, slope_threshold=1.0, rsquared_threshold=0.2)
INFOS = (("SVTYPE", "1", "String", "Type of structural variant"), ("SVLEN", ".", "Integer", "Difference in length"),
         ("END", "1", "Integer", "End position"), ("STRANDS", ".", "String", "Strand orientation"),
         ("IMPRECISE", "0", "Flag", "Imprecise structural variation"), ("CIPOS", "2", "Integer", "Confidence interval around POS"),
         ("CIEND", "2", "Integer", "Confidence interval around END"), ("CIPOS95", "2", "Integer", "95% interval, around POS"),
         ("CIEND95", "2", "Integer", "95% interval around END"), ("MATEID", ".", "String", "ID of mate breakends"),
         ("EVENT", "1", "String", "ID of event associated to breakend"), ("SECONDARY", "0", "Flag", "Secondary breakend"),
         ("SU", ".", "Integer", "Number of pieces of evidence"), ("AF", "A", "Float", "Allele Frequency"),
         ("NSAMP", "1", "Integer", "Number of samples with non-reference genotypes"))
FORMATS = (("GT", "1", "String", "Genotype"), ("CN", "1", "Float", "Copy number"), ("AB", "A", "Float", "Allele balance"))


def names(n):
    return ["S%04d" % s for s in range(n)]


def header(n, infos=INFOS, formats=FORMATS, extra=()):
    out = ["##fileformat=VCFv4.2", "##fileDate=20190101", "##reference=ref.fa", "##FILTER=<ID=LOW,Description=\"Low quality\">",
           "##contig=<ID=1,length=249250621>"]
    out += ['##INFO=<ID=%s,Number=%s,Type=%s,Description="%s">' % i for i in infos]
    out += ['##ALT=<ID=DEL,Description="Deletion">', '##ALT=<ID=DUP,Description="Duplication, tandem">']
    out += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="%s">' % f for f in formats]
    out += list(extra)
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + names(n)))
    return "\n".join(out) + "\n"


def info_of(svtype, pos, end, extra=""):
    length = end - pos if svtype == "DUP" else pos - end
    return ("SVTYPE=%s;SVLEN=%d;END=%d;STRANDS=+-:9;IMPRECISE;CIPOS=-10,9;CIEND=-8,7;CIPOS95=-2,1;CIEND95=-1,3;SU=9%s"
            % (svtype, length, end, extra))


def line(chrom, pos, ident, svtype, columns, end=None, fmt="GT:CN:AB", info=None, qual="123.45", newline=True):
    end = pos + 5000 if end is None else end
    fields = [chrom, str(pos), ident, "N", "<%s>" % svtype, qual, ".", info_of(svtype, pos, end) if info is None else info, fmt]
    return "\t".join(fields + list(columns)) + ("\n" if newline else "")


def other(chrom, pos, ident, svtype, n, newline=True):
    """a line that is no DEL or DUP: it goes through as it is, the fields the rewrite would change included"""
    alt = "N[%s:%d[" % (chrom, pos + 700) if svtype == "BND" else "<%s>" % svtype
    fields = [chrom, "%03d" % pos, ident, "N", alt, ".", "LOW", "SU=4;SVTYPE=%s;UNDECLARED=1;END=%d" % (svtype, pos + 700), "GT:AB:CN"]
    return "\t".join(fields + ["0/0:0.1:2"] * n) + ("\n" if newline else "")


def _noise(k, spread):
    """a deterministic value in [-spread, spread] with four decimals"""
    return round((((k * 2654435761) >> 7) % 2001 - 1000) / 1000.0 * spread, 4)


def cohort(n, n_pos, svtype, supported, salt=0, coarse=False):
    """n sample columns "GT:CN:AB": the first n_pos samples carry the variant (0/1 and 1/1 in turn), the others are 0/0; the CN
    follows the genotype where the call is `supported` and stays near 2 where it is not.  `coarse`: few distinct columns (the
    text of a very wide line compresses)"""
    step = {"DEL": -1.0, "DUP": 1.0}[svtype] if supported else 0.0
    gts, cns, abs_ = [], [], []
    for s in range(n):
        k = (s % 7 if coarse else s) + 31 * salt
        dose = 0 if s >= n_pos else 1 + (s % 2)
        gts.append(("0/0", "0/1", "1/1")[dose])
        cns.append("%.2f" % (2.0 + step * dose * 0.9 + _noise(k, 0.15)))
        abs_.append("%.3f" % min(max(0.03 + 0.45 * dose + _noise(k + 5, 0.03), 0.0), 1.0))
    return gts, cns, abs_


def columns(gts, cns, abs_):
    return [":".join(t) for t in zip(gts, cns, abs_)]


def genders(n, male=lambda s: s % 2 == 0, missing=()):
    return "".join("%s\t%d\n" % (name, 1 if male(s) else 2) for s, name in enumerate(names(n)) if s not in missing)


def ref_list(gts, cns, excluded=()):
    return [float(c) for s, (g, c) in enumerate(zip(gts, cns)) if g == "0/0" and s not in excluded]


def case(name, vcf, n, gender=None, exclude=None, annotation=None, slow_lines=0, low=None, error=None, kind=None, **options):
    return dict(name=name, vcf=vcf, gender=genders(n) if gender is None else gender, exclude=exclude, annotation=annotation,
                options=dict(OPTIONS, **options), slow_lines=slow_lines, low=low or {}, error=error, kind=kind, n_samples=n)


def _width_case(n):
    """a cohort of n samples: both types, both verdicts, both tests where n allows, other lines in between"""
    body, low = [], {}
    for k, (svtype, supported) in enumerate((("DEL", True), ("DEL", False), ("DUP", True), ("DUP", False))):
        for n_pos in sorted({min(n, 9), min(n, 40 + k)}):
            if n_pos == n and n > 1:
                n_pos = n - 1
            g, c, a = cohort(n, n_pos, svtype, supported, salt=k)
            if n_pos < 10:
                low[len(body)] = ref_list(g, c)
            body.append(line("1", 1000 * (len(body) + 1), "v%d" % len(body), svtype, columns(g, c, a)))
        body.append(other("1", 1000 * (len(body) + 1), "o%d" % len(body), ("BND", "INV")[k % 2], n))
    return case("width_%d" % n, header(n) + "".join(body), n, low=low)


def _columns_of(rows):
    """rows of (GT, CN, AB) strings"""
    return [":".join(r) for r in rows]


def _low_cases():
    out = []

    def one(name, svtype, refs, alts, **kw):
        rows = [("0/0", r, "0.01") for r in refs] + [(g, c, "0.5") for g, c in alts]
        n = len(rows)
        body = line("2", 5000, name, svtype, _columns_of(rows))
        out.append(case("low_" + name, header(n) + body, n, low={0: [float(r) for r in refs]}, **kw))

    one("no_ref", "DEL", [], [("0/1", "1.00")])
    one("no_alt", "DEL", ["2.00", "2.10"], [])
    one("one_ref", "DEL", ["2.00"], [("0/1", "0.90")])
    one("two_ref", "DUP", ["2.00", "2.25"], [("0/1", "3.10"), ("1/1", "4.05")])
    one("odd_ties", "DEL", ["2.00", "2.00", "2.00", "1.50", "2.50"], [("0/1", "1.20")])
    one("even_ties", "DUP", ["2.10", "2.00", "2.10", "2.00"], [("1/1", "3.70")])
    one("mad_zero_resid_half", "DEL", ["2.00", "2.00", "2.00"], [("0/1", "1.50")])          # resid 0.5 > 0.5 is false
    one("mad_zero_resid_above", "DEL", ["2.00", "2.00", "2.00"], [("0/1", "1.4375")])
    one("resid_twice_mad", "DEL", ["1.00", "2.00", "3.00"], [("0/1", "0.00")])              # resid 2.0 > 2 * 1.0 is false
    one("resid_above_twice_mad", "DEL", ["1.00", "2.00", "3.00"], [("0/1", "-0.25")])
    one("resid_half_and_twice_mad", "DUP", ["1.75", "2.00", "2.25"], [("0/1", "2.50")])
    one("quorum_half", "DEL", ["2.00", "2.05", "1.95"], [("0/1", "0.90"), ("0/1", "1.95")])  # 1 of 2 is not more than half
    one("quorum_above_half", "DEL", ["2.00", "2.05", "1.95"], [("0/1", "0.90"), ("0/1", "1.95"), ("1/1", "0.10")])
    one("other_gts", "DUP", ["2.00", "2.02"], [("0/1", "3.10"), ("1/0", "9.00"), ("0|1", "9.00"), ("./.", "9.00"), (".", "9.00")])
    one("exponent_tokens", "DEL", ["2e0", "+2.05", "195e-2", "2."], [("0/1", ".9")])
    one("long_token", "DEL", ["2.0000000000000001", "2.05"], [("0/1", "0.90")], slow_lines=1)
    # 256 reference samples, 127 below and 127 above the two middle values, which stand at samples 0 and 259: in different
    # strides of the kernel's 256 lanes, and different, so the median is (a + b) / 2 of them
    rows, k = [], 0
    for s in range(260):
        if s in (10, 11, 12, 13):
            rows.append(("0/1", "0.95", "0.5"))
        elif s in (0, 259):
            rows.append(("0/0", "2.03" if s == 0 else "2.07", "0.02"))
        else:
            rows.append(("0/0", "%.2f" % (1.0 + 0.001 * k if k < 127 else 2.5 + 0.001 * k), "0.02"))
            k += 1
    out.append(case("low_middle_in_two_strides", header(260) + line("2", 7000, "m", "DEL", _columns_of(rows)), 260,
                    low={0: [float(r[1]) for r in rows if r[0] == "0/0"]}))
    # 9 and 10 positive samples: the switch between the tests; 10 of which one is excluded
    for n_pos, excluded in ((9, None), (10, None), (10, 3)):
        g, c, a = cohort(30, n_pos, "DEL", True, salt=n_pos)
        name = "switch_%d%s" % (n_pos, "_one_excluded" if excluded is not None else "")
        skip = () if excluded is None else (excluded,)
        out.append(case(name, header(30) + line("3", 100, "s", "DEL", columns(g, c, a)), 30,
                        exclude=None if excluded is None else names(30)[excluded] + "\nNOBODY\n",
                        low={0: ref_list(g, c, skip)} if n_pos - len(skip) < 10 else {}))
    return out


def _sex_cases():
    out = []
    rows = [("0/0", "2.00", "0.01"), ("0/0", "1.01", "0.02"), ("0/1", "1.90", "0.4"), ("0/1", "2.10", "0.5"), ("0/1", "0.55", "0.5"),
            ("1/1", "0.90", "0.9"), ("1/1", "0.05", "0.9"), ("0/1", "1.00", "0.5"), ("1/1", "1.20", "1.0"), ("0/0", "2.2", "0")]
    n = len(rows)
    for name, males in (("male_majority", (1, 2, 3, 5, 6, 9)), ("female_majority", (0, 1, 7)), ("tie", (1, 2, 3, 5))):
        for chrom in ("X", "Y"):
            body = line(chrom, 300, "x1", "DEL", _columns_of(rows)) + line(chrom, 9000, "x2", "DUP", _columns_of(rows))
            out.append(case("sex_%s_%s" % (chrom, name), header(n) + body, n, gender=genders(n, lambda s: s in males)))
    g = genders(n, lambda s: s in (1, 2, 3))
    out.append(case("sex_chrX_is_autosomal", header(n) + line("chrX", 300, "x1", "DEL", _columns_of(rows)), n, gender=g,
                    low={0: [2.0, 1.01, 2.2]}))
    out.append(case("sex_other_gender_codes", header(n) + line("X", 300, "x1", "DEL", _columns_of(rows)), n,
                    gender=g.replace("S0005\t2", "S0005\t0").replace("S0002\t1", "S0002\t3")))
    # the regression on X: a male's CN counts twice
    gts, cns, abs_ = cohort(40, 24, "DEL", True, salt=4)
    cns = ["%.2f" % (float(c) / 2) if s % 2 == 0 else c for s, c in enumerate(cns)]
    out.append(case("sex_X_regression", header(40) + line("X", 300, "x1", "DEL", columns(gts, cns, abs_)), 40))
    # a sample the gender file does not name: nothing happens on an autosome, a KeyError on X
    out.append(case("sex_gender_missing_autosome", header(n) + line("4", 300, "x1", "DEL", _columns_of(rows)), n, gender=genders(n, missing=(4,)),
                    low={0: [2.0, 1.01, 2.2]}))
    out.append(case("error_gender_missing_X", header(n) + line("X", 300, "x1", "DEL", _columns_of(rows)), n, gender=genders(n, missing=(4,)),
                    error=len(header(n).splitlines()) + 1, kind="GENDER"))
    return out


def _regression_cases():
    out = []
    n = 24

    def one(name, svtype, supported, change=None, slow_lines=0, fmt="GT:CN:AB", shape=None, **kw):
        g, c, a = cohort(n, 16, shape or svtype, supported, salt=len(out))
        if change:
            change(g, c, a)
        out.append(case("high_" + name, header(n) + line("5", 800, name, svtype, columns(g, c, a) if fmt == "GT:CN:AB" else
                                                        [":".join(t) for t in zip(g, a)], fmt=fmt), n, slow_lines=slow_lines, **kw))

    def every(value, which):
        def change(g, c, a):
            (a if which == "ab" else c)[:] = [value] * n
        return change

    def first_ab(value):
        def change(g, c, a):
            a[0] = value
        return change

    one("del_kept", "DEL", True)
    one("del_split", "DEL", False)
    one("dup_kept", "DUP", True)
    one("dup_split", "DUP", False)
    one("del_wrong_sign", "DEL", True, shape="DUP")        # a DEL whose CN rises with AB: the slope's sign is flipped
    one("dup_wrong_sign", "DUP", True, shape="DEL")
    one("every_ab_missing", "DEL", True, every(".", "ab"))
    one("one_ab_minus_one", "DEL", True, first_ab("-1"))
    one("one_ab_minus_one_point", "DEL", True, first_ab("-1.0"))
    one("one_ab_missing", "DUP", True, first_ab("."))
    one("uniform_ab", "DEL", True, every("0.5", "ab"))
    one("uniform_cn", "DEL", True, every("2.00", "cn"))
    one("no_cn_in_format", "DEL", True, fmt="GT:AB")
    one("low_slope_threshold", "DEL", False, slope_threshold=-5.0, rsquared_threshold=0.0)
    one("excluded_still_regressed", "DUP", True, exclude="".join(name + "\n" for name in names(n)[16:]))
    return out


def _format_cases():
    out = []
    n = 6
    rows = [("0/0", "2.00", "0.01"), ("0/0", "2.08", "0.02"), ("0/0", "1.93", "0.0"), ("0/1", "0.95", "0.45"), ("1/1", "0.10", "0.97"), ("0/0", "2.01", "0")]
    ref = [2.0, 2.08, 1.93, 2.01]
    swapped = [":".join((g, a, c)) for g, c, a in rows]
    out.append(case("format_out_of_header_order", header(n) + line("6", 100, "f", "DEL", swapped, fmt="GT:AB:CN"), n, slow_lines=1, low={0: ref}))
    short = _columns_of(rows)
    short[1] = "0/0:2.08"
    out.append(case("format_short_sample_column", header(n) + line("6", 100, "f", "DEL", short), n, slow_lines=1, low={0: ref}))
    longer = _columns_of(rows)
    longer[2] += ":77"
    out.append(case("format_long_sample_column", header(n) + line("6", 100, "f", "DUP", longer), n, slow_lines=1, low={0: ref}))
    out.append(case("format_row_short_of_columns", header(n) + line("6", 100, "f", "DEL", _columns_of(rows)[:5]), n, slow_lines=1,
                    exclude=names(n)[5] + "\n", low={0: ref[:3]}))
    out.append(case("format_row_with_more_columns", header(n) + line("6", 100, "f", "DEL", _columns_of(rows) + ["1/1:0:1"]), n, slow_lines=1, low={0: ref}))
    out.append(case("format_gt_not_first", header(n) + line("6", 100, "f", "DEL", [":".join((c, g, a)) for g, c, a in rows], fmt="CN:GT:AB"), n, slow_lines=1))
    out.append(case("format_eight_columns", header(n) + "\t".join(line("6", 100, "f", "DEL", []).rstrip("\n").split("\t")[:8]) + "\n", n,
                    slow_lines=1, exclude="".join(name + "\n" for name in names(n))))
    # headers without the three keys of a BND pair, and with SECONDARY not a Flag
    bare = tuple(i for i in INFOS if i[0] not in ("SECONDARY", "EVENT", "MATEID"))
    typed = tuple(("SECONDARY", "1", "String", "Secondary breakend") if i[0] == "SECONDARY" else i for i in INFOS)
    unsupported = _columns_of([(g, "2.00", a) for g, _c, a in rows])
    for name, infos in (("declared", INFOS), ("undeclared", bare), ("secondary_not_a_flag", typed)):
        body = line("7", 100, "b1", "DEL", unsupported) + line("7", 900, "b2", "DUP", unsupported)
        out.append(case("header_bnd_keys_" + name, header(n, infos) + body, n, low={0: [2.0] * 4, 1: [2.0] * 4}))
    # a repeated declaration: the first wins; a Description with a comma inside its quotes
    twice = INFOS + (("SU", "1", "String", "again"), ("NOTE", "1", "String", "one, two"))
    out.append(case("header_repeated_and_quoted", header(n, twice, extra=("##source=test",)) + line("7", 100, "h", "DEL", _columns_of(rows)), n, low={0: ref}))
    # INFO items: a=b=c, a key without '=' that is no Flag, an undeclared key, a repeated key, a Flag with a value, an empty item
    info = info_of("DEL", 100, 5100, ";STRANDS=a=b=c;SU;UNDECLARED=7;AF=0.1;AF=0.25;IMPRECISE=1;;NSAMP=2")
    out.append(case("info_items", header(n) + line("8", 100, "i", "DEL", _columns_of(rows), info=info) + line("8", 100, "i2", "DUP", unsupported, info=info), n,
                    low={0: ref, 1: [2.0] * 4}))
    # QUAL: '.', an integer, an exponent; POS with a leading zero (rewritten by int())
    body = line("8", 100, "q1", "DEL", _columns_of(rows), qual=".") + line("8", 200, "q2", "DEL", _columns_of(rows), qual="7") + \
        line("8", 300, "q3", "DEL", _columns_of(rows), qual="1.5e2").replace("\t300\t", "\t0300\t")
    out.append(case("qual_and_pos", header(n) + body, n, low={0: ref, 1: ref, 2: ref}))
    # SVTYPE twice: the first decides whether the line is looked at, the last what becomes of it
    twice_info = info_of("DEL", 100, 5100, ";SVTYPE=BND")
    body = line("8", 100, "t1", "DEL", _columns_of(rows), info=twice_info) + line("8", 200, "t2", "DEL", unsupported, info=info_of("DEL", 200, 5200, ";SVTYPE=DUP"))
    out.append(case("svtype_twice", header(n) + body, n, slow_lines=2, low={1: [2.0] * 4}))
    # other lines between, in front and behind; the last line without its newline, as it is and rewritten
    mixed = other("9", 50, "o1", "INV", n) + line("9", 100, "d1", "DEL", _columns_of(rows)) + other("9", 150, "o2", "BND", n) + \
        line("9", 200, "d2", "DUP", unsupported)
    out.append(case("last_line_verbatim_bare", header(n) + mixed + other("9", 300, "o3", "INV", n, newline=False), n, low={1: ref, 3: [2.0] * 4}))
    out.append(case("last_line_rewritten_bare", header(n) + mixed + line("9", 400, "d3", "DEL", _columns_of(rows), newline=False), n,
                    low={1: ref, 3: [2.0] * 4, 4: ref}))
    out.append(case("trailing_blanks", header(n) + line("9", 400, "d3", "DEL", _columns_of(rows)).rstrip("\n") + " \t\n" + other("9", 500, "o", "BND", n), n,
                    low={0: ref}))
    out.append(case("no_body", header(n), n))
    out.append(case("no_header_samples", "##fileformat=VCFv4.1\n" + other("9", 50, "o1", "INV", 0), 0))
    return out


def _annotation_cases():
    n = 6
    rows = [("0/0", "2.00", "0.01"), ("0/0", "2.08", "0.02"), ("0/0", "1.93", "0.0"), ("0/1", "0.95", "0.45"), ("1/1", "0.10", "0.97"), ("0/0", "2.01", "0")]
    cols = _columns_of(rows)
    ref = [2.0, 2.08, 1.93, 2.01]
    bed = "".join("\t".join(map(str, f)) + "\n" for f in (
        ("1", 1000, 2000, "SINE|Alu|AluY"), ("1", 5000, 5450, "LINE|L1|L1HS"), ("1", 5400, 6000, "LINE|L1|L1HS"), ("1", 5100, 5950, "DNA|x|SVA_D"),
        ("1", 9000, 9899, "SINE|Alu|AluJ"), ("1", 12000, 13000, "LTR|ERV|HERV"), ("1", 12000, 12990, "Satellite"), ("short", 1, 2),
        ("1", 20000, 21000, "Retroposon|SVA|SVA_F"), ("1", 30000, 31000, "SINE|late"), ("1", 25000, 26000, "SINE|behind_a_later_start"),
        ("2", 100, 5100, "SINE|other_contig")))
    body = "".join([
        line("1", 1000, "a_sine_hit", "DEL", cols, end=2000), line("1", 1000, "a_sine_at_0.9", "DEL", cols, end=2111),
        line("1", 1000, "a_miss_under_0.9", "DEL", cols, end=2112), line("1", 5000, "a_collapse_two_classes", "DEL", cols, end=6000),
        line("1", 12000, "a_not_me", "DEL", cols, end=13000), line("1", 20000, "a_sva", "DEL", cols, end=21000),
        line("1", 1000, "a_dup_is_not_annotated", "DUP", cols, end=2000), line("1", 25000, "a_sweep_ended", "DEL", cols, end=26000),
        line("1", 9000, "a_second_look", "DEL", cols, end=9900), line("3", 100, "a_no_contig", "DEL", cols, end=5100),
        line("1", 700, "a_empty", "DEL", cols, end=700), other("1", 1000, "o", "BND", n)])
    low = {k: ref for k in (2, 6, 7, 9, 10)}
    out = [case("annotation", header(n) + body, n, annotation=bed, low=low),
           case("annotation_fraction_0.5", header(n) + body, n, annotation=bed, low={k: ref for k in (6, 7, 9, 10)}, f_overlap=0.5)]
    # an MEI line in front of a line that cannot be tested: the annotation comes before the depth tests
    bad = line("1", 1000, "mei_with_bad_cn", "DEL", _columns_of([("0/0", "two", "0")] + rows[1:]), end=2000)
    out.append(case("annotation_before_depth", header(n) + bad + line("1", 40000, "d", "DEL", cols), n, annotation=bed, low={1: ref}))
    # a DEL without END on a contig the BED does not hold is never asked for it (kept: a kept line needs no END); a line that
    # starts as a DUP and ends as a DEL is annotated
    no_end = line("3", 100, "no_end", "DEL", cols, info="SVTYPE=DEL;SVLEN=-5000;SU=9")
    dup_del = line("1", 1000, "dup_then_del", "DUP", cols, end=2000, info=info_of("DUP", 1000, 2000, ";SVTYPE=DEL"))
    out.append(case("annotation_end_and_last_svtype", header(n) + no_end + dup_del, n, annotation=bed, low={0: ref}))
    # the lines in front of the one the run ends on are written first, and an earlier error of the depth tests comes first
    first = len(header(n).splitlines()) + 1
    good, bad_cn = line("1", 40000, "d", "DEL", cols), line("1", 41000, "e", "DUP", _columns_of([("0/0", "abc", "0")] + rows[1:]))
    bad_pos = line("1", 3, "p", "DEL", cols, end=2000).replace("\t3\t", "\t3x\t")
    out.append(case("error_annotation_depth_error_in_front", header(n) + good + bad_cn + bad_pos, n, annotation=bed, error=first + 1, kind="NUMBER"))
    out.append(case("error_annotation_pos_behind_a_good_line", header(n) + good + bad_pos + good, n, annotation=bed, error=first + 1, kind="POS"))
    out.append(case("error_annotation_del_without_end", header(n) + good + line("1", 100, "no_end", "DEL", cols, info="SVTYPE=DEL;SVLEN=-5000;SU=9"), n,
                    annotation=bed, error=first + 1, kind="KEY"))
    out.append(case("error_annotation_class_without_fields", header(n) + line("1", 12000, "e", "DEL", cols, end=12990), n,
                    annotation="1\t12000\t12990\tSatellite\n", error=len(header(n).splitlines()) + 1))
    return out


def _error_cases():
    n = 6
    rows = [("0/0", "2.00", "0.01"), ("0/0", "2.08", "0.02"), ("0/0", "1.93", "0.0"), ("0/1", "0.95", "0.45"), ("1/1", "0.10", "0.97"), ("0/0", "2.01", "0")]
    cols = _columns_of(rows)
    unsupported = _columns_of([(g, "2.00", a) for g, _c, a in rows])
    first = len(header(n).splitlines()) + 1
    good = line("1", 10, "ok", "DEL", cols)
    out = []

    def one(name, kind, bad_line, **kw):
        out.append(case("error_" + name, header(n) + good + bad_line + good, n, error=first + 1, kind=kind, **kw))

    one("cn_no_number", "NUMBER", line("1", 20, "e", "DEL", _columns_of([rows[0], ("0/0", "abc", "0")] + rows[2:])))
    one("cn_dot", "NUMBER", line("1", 20, "e", "DUP", _columns_of([rows[0], ("./.", ".", ".")] + rows[2:])))
    one("no_cn_low", "KEY", line("1", 20, "e", "DEL", [":".join((g, a)) for g, _c, a in rows], fmt="GT:AB"))
    one("sample_without_cn", "KEY", line("1", 20, "e", "DEL", ["0/0"] + cols[1:]))
    one("bnd_without_end", "KEY", line("1", 20, "e", "DEL", unsupported, info="SVTYPE=DEL;SVLEN=-9;CIPOS=0,0;CIEND=0,0;CIPOS95=0,0;CIEND95=0,0"))
    one("bnd_without_svlen", "KEY", line("1", 20, "e", "DUP", unsupported, info="SVTYPE=DUP;END=99;CIPOS=0,0;CIEND=0,0;CIPOS95=0,0;CIEND95=0,0"))
    one("bnd_without_ciend95", "KEY", line("1", 20, "e", "DUP", unsupported, info="SVTYPE=DUP;END=99;SVLEN=79;CIPOS=0,0;CIEND=0,0;CIPOS95=0,0"))
    one("undeclared_format_key", "FORMAT", line("1", 20, "e", "DEL", [c + ":5" for c in cols], fmt="GT:CN:AB:DP"))
    one("seven_columns", "COLUMNS", "1\t20\te\tN\t<DEL>\t.\t.\n")
    one("pos_no_integer", "POS", line("1", 20, "e", "DEL", cols).replace("\t20\t", "\t2x\t"))
    one("qual_no_number", "QUAL", line("1", 20, "e", "DEL", cols, qual="high"))
    # the regression: an AB that is no number, a sample without AB; excluded samples are read all the same
    g, c, a = cohort(24, 16, "DEL", True, salt=2)
    for name, change in (("ab_no_number", lambda a: a.__setitem__(20, "x")), ("ab_empty", lambda a: a.__setitem__(23, ""))):
        a2 = list(a)
        change(a2)
        out.append(case("error_" + name, header(24) + line("1", 20, "e", "DEL", columns(g, c, a2)), 24, error=len(header(24).splitlines()) + 1, kind="NUMBER",
                        exclude=names(24)[20] + "\n" + names(24)[23] + "\n"))
    out.append(case("error_sample_without_ab", header(24) + line("1", 20, "e", "DEL", [":".join(t) for t in zip(g, c)], fmt="GT:CN"), 24,
                    error=len(header(24).splitlines()) + 1, kind="KEY"))
    return out


def _capacity_case():
    n = CAPACITY + 1
    body = []
    for svtype, supported, n_pos in (("DEL", True, 8), ("DUP", False, 700)):
        body.append(line("1", 1000 * (len(body) + 1), "w%d" % len(body), svtype, columns(*cohort(n, n_pos, svtype, supported, coarse=True))))
    g, c, _a = cohort(n, 8, "DEL", True, coarse=True)
    return case("width_above_capacity", header(n) + "".join(body), n, slow_lines=2, low={0: ref_list(g, c)})


def cases():
    out = [_width_case(n) for n in SAMPLE_COUNTS]
    out += _low_cases() + _sex_cases() + _regression_cases() + _format_cases() + _annotation_cases() + _error_cases()
    out.append(_capacity_case())
    assert len({c["name"] for c in out}) == len(out)
    return out


def near_case():
    """not in the goldens: a regression whose slope is exactly its threshold (two points per dose, CN = 2 - AB on a DEL): the
    line is flagged SVT_CLASSIFY_NEAR"""
    rows = [("0/1", "1.50", "0.50"), ("1/1", "1.00", "1.00")] * 6 + [("0/0", "2.00", "0.00")] * 4
    return case("near_slope", header(16) + line("1", 100, "n", "DEL", _columns_of(rows)), 16)


def bcf_case():
    """not in the goldens: 65 samples on the contig the header declares, every field within what a BCF record holds; both tests,
    both verdicts, out of order"""
    body = []
    for k, (svtype, supported, n_pos) in enumerate((("DEL", True, 9), ("DUP", False, 30), ("DEL", False, 5), ("DUP", True, 31), ("DEL", True, 40))):
        body.append(line("1", 90000 - 7000 * k, "b%d" % k, svtype, columns(*cohort(65, n_pos, svtype, supported, salt=k))))
    return case("bcf_65", header(65) + "".join(body), 65)


def nonfinite_cases():
    """not in the goldens (a departure): a CN or AB that float() reads as nan or inf"""
    rows = [("0/0", "2.00", "0.01"), ("0/0", "nan", "0.02"), ("0/1", "0.95", "0.45")]
    g, c, a = cohort(24, 16, "DEL", True)
    a[5] = "inf"
    return [case("nonfinite_cn", header(3) + line("1", 100, "n", "DEL", _columns_of(rows)), 3, error=len(header(3).splitlines()) + 1),
            case("nonfinite_ab", header(24) + line("1", 100, "n", "DEL", columns(g, c, a)), 24, error=len(header(24).splitlines()) + 1)]


def write_case(c, directory):
    """the case's files under `directory`: (vcf, gender, exclude or None, annotation or None)"""
    import os
    paths = []
    for key, name in (("vcf", "cohort.vcf"), ("gender", "genders.tsv"), ("exclude", "exclude.txt"), ("annotation", "elements.bed")):
        if c[key] is None:
            paths.append(None)
            continue
        paths.append(os.path.join(directory, name))
        with open(paths[-1], "w", newline="") as f:
            f.write(c[key])
    return tuple(paths)

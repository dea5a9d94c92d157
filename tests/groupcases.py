"""The corpus of svtyper_amd.group_multiline: synthetic VCFs with BND pairs, shared by tests/test_group_host.py,
tests/test_group_native.py, tests/test_group_device.py and tests/golden/make_golden_group.py.  Everything is built in code and
deterministic; inputs are not stored.

A case: name, vcf, n_samples, and what the case was built for: slow_lines (the lines outside the envelope of
svtyper_amd/csrc/svt_vcf_group.h, which the host's plain C++ decides, exactly), irregular (the file is not regular in the sense
of DESIGN 3.4, so the device hands the join to the host), error (None, or the 1-based line of the VCF that ends the run) and kind
(of an error: which SVT_GROUP_BAD_* the native code names it by, as the name behind that prefix; None for the one error that is
Python's, a body line without a #CHROM line in front).  What the reference's script gives for a case is in
tests/golden/group_cases.json.gz, by name.

The generator of the goldens runs the script under Python 3: tokens on which Python 2 and 3 disagree (underscores in numbers,
digits outside ASCII, blanks outside ASCII) stay out of the corpus.
"""
SORT_TILE = 1024                                    # svtyper_amd/csrc/svt_radix_sort_kernel.h: kSortTile, elements
PAIR_COUNTS = (1, 2, 63, 64, 65, 257, SORT_TILE // 2 + 1)
INFOS = (("SVTYPE", "1", "String", "Type of structural variant"), ("END", "1", "Integer", "End position"),
         ("STRANDS", ".", "String", "Strand orientation"), ("IMPRECISE", "0", "Flag", "Imprecise structural variation"),
         ("CIPOS", "2", "Integer", "Confidence interval around POS"), ("CIEND", "2", "Integer", "Confidence interval around END"),
         ("MATEID", ".", "String", "ID of mate breakends"), ("SU", ".", "Integer", "Number of pieces of evidence"))
FORMATS = (("GT", "1", "String", "Genotype"), ("SU", "1", "Integer", "Supporting evidence"), ("GQ", "1", "Integer", "declared with another type"),
           ("AP", "A", "Integer", "Alternate allele paired-end observations"))
FORMAT = "GT:SU:GQ:AP"
OTHER = "SVTYPE=%s;END=%d;STRANDS=+-:4;IMPRECISE;CIPOS=-10,9;CIEND=-5,0;SU=4;UNDECLARED=1"
BND = "SVTYPE=BND;MATEID=%s;STRANDS=+-:3;CIPOS=-3,3;CIEND=0,0;SU=3"
SVTYPES = ("DEL", "DUP", "INV", "INS")


def names(n):
    return ["S%04d" % s for s in range(n)]


def header(n, infos=INFOS, formats=FORMATS, chrom=True):
    out = ["##fileformat=VCFv4.2", "##fileDate=20190101", "##reference=ref.fa", "##FILTER=<ID=LOW,Description=\"Low quality\">",
           "##contig=<ID=1,length=249250621>", "##source=test"]
    out += ['##INFO=<ID=%s,Number=%s,Type=%s,Description="%s">' % i for i in infos]
    out += ['##ALT=<ID=DEL,Description="Deletion">', '##ALT=<ID=DUP,Description="Duplication, tandem">']
    out += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="%s">' % f for f in formats]
    if chrom:
        out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] + (["FORMAT"] + names(n) if n else [])))
    return "\n".join(out) + "\n"


def columns(n, salt=0):
    return ["%s:%d:%d:%d" % (("0/0", "0/1", "1/1", "./.")[(s + salt) % 4], (3 * s + salt) % 17, (7 * s + 5 * salt) % 99, (s + 2 * salt) % 11)
            for s in range(n)]


def line(n, pos, ident, info, alt="<DEL>", qual="12.5", chrom="1", filt=".", fmt=FORMAT, cols=None, salt=0):
    fields = [chrom, str(pos), ident, "N", alt, qual, filt, info]
    if n or cols is not None:
        fields += [fmt] + (columns(n, salt) if cols is None else list(cols))
    return "\t".join(fields) + "\n"


def other(n, pos, ident, svtype="DEL", **kw):
    return line(n, pos, ident, OTHER % (svtype, pos + 500), alt="<%s>" % svtype, **kw)


def bnd(n, pos, ident, mate, **kw):
    kw.setdefault("alt", "N[2:%d[" % (pos + 7))
    return line(n, pos, ident, BND % mate, **kw)


def case(name, vcf, n, slow_lines=0, irregular=False, error=None, kind=None):
    return dict(name=name, vcf=vcf, n_samples=n, slow_lines=slow_lines, irregular=irregular, error=error, kind=kind)


def pairs_body(n, n_pairs, apart=True):
    """n_pairs pairs, every first mate in the front half and every second in the back half (`apart`) or side by side, lines of
    every other SVTYPE between them"""
    first, second = [], []
    for k in range(n_pairs):
        a = bnd(n, 1000 + k, "p%d_1" % k, "p%d_2" % k, qual="%d.25" % k, salt=k)
        b = bnd(n, 5000 + k, "p%d_2" % k, "p%d_1" % k, qual=".", filt="LOW", salt=k + 1, alt="]1:%d]N" % k)
        filler = other(n, 100 + k, "o%d" % k, SVTYPES[k % 4], salt=k) if k % 3 == 0 else ""
        if apart:
            first.append(a + filler)
            second.append(b if k % 5 else b + filler.replace("\to%d\t" % k, "\tq%d\t" % k))
        else:
            first.append(a + b + filler)
    return "".join(first) + "".join(reversed(second))


def _regular_cases():
    n = 2
    out = [case("pairs_%d" % k, header(n) + pairs_body(n, k), n) for k in PAIR_COUNTS]
    out.append(case("no_bnd", header(n) + "".join(other(n, 10 * k, "o%d" % k, SVTYPES[k % 4], salt=k) for k in range(9)), n))
    out.append(case("mates_adjacent", header(n) + pairs_body(n, 5, apart=False), n))
    body = bnd(n, 1, "a", "b") + "".join(other(n, 10 + k, "o%d" % k, SVTYPES[k % 4]) for k in range(7)) + bnd(n, 2, "b", "a", qual="99")
    out.append(case("mates_first_and_last", header(n) + body, n))
    body = bnd(n, 1, "u0", "nobody") + bnd(n, 2, "a", "b") + bnd(n, 3, "u1", "gone") + bnd(n, 4, "b", "a") + bnd(n, 5, "c", "d") + \
        bnd(n, 6, "u2", "u3x") + bnd(n, 7, "d", "c") + bnd(n, 8, "u3", "u2x")
    out.append(case("unpaired_around_pairs", header(n) + body, n))
    out.append(case("unpaired_only", header(n) + bnd(n, 1, "u0", "x") + bnd(n, 2, "u1", "y") + bnd(n, 3, "u2", "u1_"), n))
    body = other(n, 5, "a", "DEL") + bnd(n, 6, "x", "a") + other(n, 7, "y", "DUP") + bnd(n, 8, "z", "y") + bnd(n, 9, "y2", "z2")
    out.append(case("other_line_with_a_mateid_as_id", header(n) + body, n))
    return out


def _shape_cases():
    out = []
    n = 1
    body = ""
    for k, size in enumerate((1, 15, 16, 17, 64)):
        a, b = "A" * size, "B" * (size - 1) + "x"
        body += bnd(n, 10 + k, a, b) + other(n, 50 + k, "o" * size) + bnd(n, 90 + k, b, a, qual="7")
    body += bnd(n, 200, "", "e") + bnd(n, 201, "e", "")
    out.append(case("id_lengths", header(n) + body, n))
    body = "".join(bnd(n, 10 + k, "r%d_a" % k, "r%d_b" % k, chrom="c" * (k + 1)) for k in range(16))
    body += "".join(bnd(n, 40 + k, "r%d_b" % k, "r%d_a" % k, chrom="d" * (16 - k)) for k in range(16))
    out.append(case("id_at_every_residue", header(n) + body, n))
    for n in (0, 3):
        body = other(n, 5, "o") + bnd(n, 6, "a", "b", qual=".") + other(n, 7, "i", "INS", qual=".") + bnd(n, 8, "b", "a", qual="3")
        out.append(case("samples_%d" % n, header(n) + body, n))
    n = 3
    eight = "\t".join(other(n, 5, "e").split("\t")[:8]) + "\n"
    eight_bnd = "\t".join(bnd(n, 6, "a", "b").split("\t")[:8]) + "\n"
    out.append(case("eight_columns", header(n) + eight + eight_bnd + other(n, 7, "o") + bnd(n, 8, "b", "a"), n))
    out.append(case("last_line_bare", header(n) + bnd(n, 6, "a", "b") + bnd(n, 8, "b", "a").rstrip("\n"), n))
    out.append(case("carriage_returns", header(n).replace("\n", "\r\n") + (bnd(n, 6, "a", "b") + bnd(n, 8, "b", "a")).replace("\n", "\r\n"), n))
    a = bnd(n, 6, "a", "b", qual="1.005", fmt="GT:AP", cols=["0/1:4", "1/1:5", "./.:6"])
    b = bnd(n, 8, "b", "a", qual="77", filt="LOW", fmt="GT:SU:GQ", cols=["0/0:1:2", "0/0:3:4", "0/0:5:6"])
    out.append(case("mate_takes_the_first_ones_samples", header(n) + a + other(n, 7, "o") + b, n))
    info = "SVTYPE=BND;MATEID=wrong;MATEID=b=c;CIPOS=x;CIPOS=1,2=y;;SU;STRANDS=a=b"
    out.append(case("info_dictionary", header(n) + line(n, 6, "a", info, alt="N[") + line(n, 8, "b", info.replace("=b=c", "=a"), alt="[N"), n))
    a = bnd(n, 6, "a", "b", fmt="GT:AP:SU", cols=["0/1:4:1", "1/1:5:2", "./.:6:3"])
    out.append(case("format_out_of_order_on_the_first", header(n) + a + bnd(n, 8, "b", "a"), n, slow_lines=1))
    return out


def _irregular_cases():
    n = 1
    out = []

    def one(name, body):
        out.append(case(name, header(n) + body, n, irregular=True))

    one("duplicate_id_overwritten", bnd(n, 1, "a", "b", qual="1") + bnd(n, 2, "a", "b", qual="2") + bnd(n, 3, "b", "a"))
    one("duplicate_id_paired_twice", bnd(n, 1, "a", "b") + bnd(n, 2, "b", "a", qual="2") + bnd(n, 3, "b", "a", qual="3"))
    one("third_line_names_a_stored_id", bnd(n, 1, "a", "b") + bnd(n, 2, "b", "a") + other(n, 3, "o") + bnd(n, 4, "c", "a"))
    one("chain", bnd(n, 1, "a", "b") + bnd(n, 2, "b", "c") + bnd(n, 3, "c", "a") + bnd(n, 4, "a2", "c"))
    one("self_mate_alone", bnd(n, 1, "a", "a") + other(n, 2, "o"))
    one("self_mate_doubled", bnd(n, 1, "a", "a", qual="1") + bnd(n, 2, "a", "a", qual="2") + bnd(n, 3, "a", "a", qual="3"))
    one("two_dot_ids", bnd(n, 1, ".", "x") + bnd(n, 2, ".", "y") + bnd(n, 3, "z", "."))
    return out


def _refusal_cases():
    """one line per reason the rule leaves a line to the plain C++ (SVT_GROUP_SLOW_*), none of which ends the run"""
    n = 1
    out = []

    def one(name, marked):
        out.append(case("refused_" + name, header(n) + bnd(n, 1, "a", "b") + marked + bnd(n, 3, "b", "a") + other(n, 4, "o"), n, slow_lines=1))

    one("head_pos_signed", other(n, 2, "m").replace("\t2\t", "\t+2\t"))
    one("head_qual_blanks", other(n, 2, "m", qual=" 8 "))
    one("format_gt_not_first", other(n, 2, "m", fmt="SU:GT", cols=["3:0/1"]))
    one("bare_end", line(n, 2, "m", "SVTYPE=DEL;END;CIPOS=0,0;CIEND=0,0"))
    one("bare_svtype", line(n, 2, "m", "SVTYPE;END=9;CIPOS=0,0;CIEND=0,0"))
    one("bare_mateid", line(n, 2, "m", "SVTYPE=BND;MATEID;CIPOS=0,0", alt="N["))
    one("token_signed_and_blank", line(n, 2, "m", "SVTYPE=DEL;END= 12 ;CIPOS=+3, 4;CIEND=-0,0012345678"))
    one("token_ten_digits", line(n, 2, "m", "SVTYPE=DEL;END=1234567890;CIPOS=0,0;CIEND=0,0"))
    one("token_of_an_unpaired_bnd", line(n, 2, "m", "SVTYPE=BND;MATEID=q;CIPOS=x,y", alt="N["))
    one("alt_empty_unpaired", bnd(n, 2, "m", "q", alt=""))
    return out


def _error_cases():
    n = 2
    out = []
    good = [other(n, 10, "g0"), bnd(n, 11, "g1", "g2"), bnd(n, 12, "g2", "g1")]
    first = len(header(n).splitlines()) + 1

    def one(name, kind, bad, slow_lines=0, stored=""):
        """`bad` in front of, between and behind lines that are written; `stored`: a line in front of it that is only stored"""
        for where, front, behind in (("first", [], good), ("middle", good[:1], good[1:]), ("last", good, [])):
            body = "".join(front) + stored + bad + "".join(behind)
            out.append(case("error_%s_%s" % (name, where), header(n) + body, n, slow_lines=slow_lines, kind=kind,
                            error=first + len(front) + len(stored.splitlines())))

    one("no_svtype", "KEY", line(n, 20, "e", "END=30;CIPOS=0,0;CIEND=0,0"))
    one("bnd_without_mateid", "KEY", line(n, 20, "e", "SVTYPE=BND;CIPOS=0,0", alt="N["))
    one("no_end", "KEY", line(n, 20, "e", "SVTYPE=DEL;CIPOS=0,0;CIEND=0,0"))
    one("no_cipos", "KEY", line(n, 20, "e", "SVTYPE=DUP;END=30;CIEND=0,0"))
    one("no_ciend", "KEY", line(n, 20, "e", "SVTYPE=INS;END=30;CIPOS=0,0"))
    one("end_no_integer", "NUMBER", line(n, 20, "e", "SVTYPE=DEL;END=3.0;CIPOS=0,0;CIEND=0,0"), slow_lines=1)
    one("cipos_no_integer", "NUMBER", line(n, 20, "e", "SVTYPE=DEL;END=30;CIPOS=0,;CIEND=0,0"), slow_lines=1)
    one("ciend_no_integer", "NUMBER", line(n, 20, "e", "SVTYPE=DEL;END=30;CIPOS=0,0;CIEND=a,0"), slow_lines=1)
    one("bare_cipos", "BARE", line(n, 20, "e", "SVTYPE=DEL;END=30;CIPOS;CIEND=0,0"), slow_lines=1)
    one("bare_ciend", "BARE", line(n, 20, "e", "SVTYPE=DEL;END=30;CIPOS=1,1;CIEND"), slow_lines=1)
    mate = line(n, 21, "f", "SVTYPE=BND;MATEID=e;CIPOS=0,0", alt="N[")
    one("pair_cipos_missing_on_the_first", "KEY", mate, stored=line(n, 20, "e", "SVTYPE=BND;MATEID=f", alt="N["))
    one("pair_cipos_missing_on_the_second", "KEY", line(n, 21, "f", "SVTYPE=BND;MATEID=e", alt="N["),
        stored=line(n, 20, "e", "SVTYPE=BND;MATEID=f;CIPOS=0,0", alt="N["))
    one("pair_cipos_no_integer_on_the_first", "NUMBER", mate, slow_lines=1, stored=line(n, 20, "e", "SVTYPE=BND;MATEID=f;CIPOS=0.5,1", alt="N["))
    one("pair_alt_empty", "ALT", mate, slow_lines=1, stored=line(n, 20, "e", "SVTYPE=BND;MATEID=f;CIPOS=0,0", alt=""))
    one("undeclared_format_key", "FORMAT", other(n, 20, "e", fmt=FORMAT + ":XX", cols=[c + ":5" for c in columns(n)]), slow_lines=1)
    one("seven_columns", "EIGHT", "1\t20\te\tN\t<DEL>\t.\t.\n", slow_lines=1)
    one("one_column", "COLUMNS", "1\n", slow_lines=1)
    one("pos_no_integer", "POS", other(n, 20, "e").replace("\t20\t", "\t2x\t"), slow_lines=1)
    one("qual_no_number", "QUAL", other(n, 20, "e", qual="high"), slow_lines=1)
    out.append(case("error_no_chrom_line", header(n, chrom=False) + good[0], n, error=len(header(n, chrom=False).splitlines()) + 1, kind=None))
    return out


def cases():
    out = _regular_cases() + _shape_cases() + _irregular_cases() + _refusal_cases() + _error_cases()
    assert len({c["name"] for c in out}) == len(out)
    return out


def bcf_case():
    """not in the goldens: pairs on the contig the header declares, every field within what a BCF record holds"""
    return case("bcf_pairs", header(2) + pairs_body(2, 5).replace(";UNDECLARED=1", ""), 2)


def write_case(c, directory):
    """the case's VCF under `directory`: its path"""
    import os
    path = os.path.join(directory, "calls.vcf")
    with open(path, "w", newline="") as f:
        f.write(c["vcf"])
    return path

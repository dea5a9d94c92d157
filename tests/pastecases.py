"""The corpus of svtyper_amd.paste: per-sample VCFs to join, shared by tests/test_paste_host.py, tests/test_paste_native.py,
tests/test_paste_device.py and tests/golden/make_golden_paste.py.

Every input is derived deterministically from tests/data/example.gt.vcf (one sample) and tests/golden/three.gt.vcf.gz (three):
the samples renamed, GT, SQ and QUAL varied by (input, line).  The master keeps a cut of the fixture's header (one INFO
declaration dropped, so that its key is undeclared in the body); an input's header is a ##fileformat line and its #CHROM line,
which is all the join reads of it.

A case: name, master (text or None: a second handle on the first input), inputs (texts), sum_quals, afreq, and what the case was
built for: slow_lines (body lines outside the envelope of svtyper_amd/csrc/svt_vcf_paste.h that still have output bytes: the
host's slow path writes them) and error (None, or file -- 0 the master, k input k - 1 --, the 1-based line of that file, and
whether the reference prints a message instead of a traceback).  What the reference's scripts give for a case is in
tests/golden/paste_cases.json.gz, by name.
"""
import gzip
import os

HERE = os.path.dirname(os.path.abspath(__file__))
INPUT_COUNTS = (1, 2, 3, 63, 64, 65, 130)
DROPPED_INFO = "EVENT"                               # in the body, not in the master's header
KEPT_KEYS = ("##fileformat", "##fileDate", "##reference", "##INFO", "##ALT", "##FORMAT", "##FILTER", "##contig")
GTS = ("0/0", "0/1", "1/1", "0/1", "0/0")


def _split(text):
    lines = text.splitlines()
    return [l for l in lines if l.startswith("##")], [l for l in lines if not l.startswith("#")]


def _sources():
    with open(os.path.join(HERE, "data", "example.gt.vcf")) as f:
        one = _split(f.read())
    with gzip.open(os.path.join(HERE, "golden", "three.gt.vcf.gz"), "rt") as f:
        three = _split(f.read())
    return one, three


def master_header(header, contigs=8):
    out, seen = [], 0
    for line in header:
        key = line.split("=")[0]
        if key not in KEPT_KEYS or line.startswith("##INFO=<ID=%s," % DROPPED_INFO):
            continue
        if key == "##contig":
            seen += 1
            if seen > contigs:
                continue
        out.append(line)
    return out


def sample_column(column, s, j, gt=None):
    """the fixture's sample column with the GT and SQ of (input s, line j)"""
    fields = column.split(":")
    fields[0] = gt if gt is not None else GTS[(s * 7 + j * 3) % len(GTS)]
    fields[5] = qual_of(s, j)
    return ":".join(fields)


def qual_of(s, j):
    return "%.2f" % ((s * 13 + j * 29) % 500 + 0.25 * (s % 4))


def build(name, n, lines, sum_quals, afreq, own_master, body, edit=None, slow_lines=0, error=None, extra_samples=None, bare_info=False,
          contigs=False, sites_only_header=False):
    """`body`: the fixture's body lines to use; `edit(s, j, columns)`: the case's own changes to input s's line j (s = -1: the
    master's), returning the columns; `extra_samples`: {s: a second sample column's source} for an input with two samples;
    `sites_only_header`: the master's #CHROM line ends with INFO (the pasted header then has no FORMAT column: the reference's bytes)"""
    (one_header, _one_body), (three_header, _three_body) = _sources()
    header = master_header(three_header if contigs else one_header)
    master_lines, inputs = [], [[] for _ in range(n)]
    for j, line in enumerate(body[:lines]):
        columns = line.split("\t")
        base = columns[:9]
        m = list(base[:8])
        if edit:
            m = edit(-1, j, m)
        master_lines.append("\t".join(m))
        for s in range(n):
            c = list(base)
            c[5] = qual_of(s, j)
            if bare_info:
                c[7] = "."
            c.append(sample_column(columns[9], s, j))
            if extra_samples and s in extra_samples:
                c.append(sample_column(columns[9], s + 1000, j, gt="0|1"))
            if edit:
                c = edit(s, j, c)
            inputs[s].append("\t".join(c))
    chrom = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"
    texts = []
    for s in range(n):
        names = ["S%03d" % s] + (["S%03db" % s] if extra_samples and s in extra_samples else [])
        texts.append("##fileformat=VCFv4.2\n" + chrom + "\tFORMAT\t" + "\t".join(names) + "\n" + "".join(l + "\n" for l in inputs[s]))
    if own_master:
        master = "\n".join(header) + "\n" + chrom + ("" if sites_only_header else "\tFORMAT") + "\n" + "".join(l + "\n" for l in master_lines)
    else:                                           # the first input is the master: it carries the header
        master = None
        texts[0] = "\n".join(header) + "\n" + texts[0].split("\n", 1)[1]
    return dict(name=name, master=master, inputs=texts, sum_quals=sum_quals, afreq=afreq, slow_lines=slow_lines, error=error)


def _set(columns, index, value):
    columns = list(columns)
    columns[index] = value
    return columns


def _gt(columns, gt, sample=9):
    fields = columns[sample].split(":")
    fields[0] = gt
    return _set(columns, sample, ":".join(fields))


def cases():
    (_h1, one), (_h3, three) = _sources()
    out = []
    # the four ways to name the master and the QUAL, at N = 1, 2, 3
    out.append(build("n1_first_is_master", 1, 5, False, False, False, one))
    out.append(build("n1_first_is_master_q", 1, 6, True, False, False, one))
    out.append(build("n2_master", 2, 7, False, False, True, one, sites_only_header=True))

    def tenths(s, j, c):                            # 0 + 0.1 + 0.2: repr says 0.30000000000000004, %.12g says 0.3
        if j == 2:
            return _set(c, 5, "0" if s < 0 else ("0.1", "0.2")[s])
        if j == 3 and s == 1:                       # an input's line with trailing blanks
            return _set(c, 9, c[9] + " \t ")
        return c
    out.append(build("n2_master_q_tenths", 2, 7, True, False, True, one, edit=tenths))

    def shapes(s, j, c):
        if j == 0 and s >= 0:
            return _gt(c, ("0|1", "1|1", "1|0")[s])             # phased
        if j == 1 and s >= 0:
            return _gt(c, ("./.", "0/1", ".")[s])               # no call
        if j == 2 and s >= 0:
            return _gt(c, ("1", "0", "1")[s])                   # haploid
        if j == 3:                                              # two ALTs
            c = _set(c, 4, "<DEL>,<DUP>")
            return c if s < 0 else _gt(c, ("1/2", "0/2", "2/2")[s])
        if j == 4 and s == 2:
            return c[:9]                                        # exactly nine columns
        if j == 5 and s == 0:
            return _set(c, 9, c[9] + "  ")                      # trailing blanks
        if j == 6 and s <= 0:                                   # a flag, an undeclared key (EVENT), a value with two '='
            return _set(c, 7, c[7] + ";IMPRECISE;TOOL=LUM=PY")
        return c
    for q in (False, True):
        out.append(build("n3_afreq_shapes" + ("_q" if q else ""), 3, 9, q, True, not q, one, edit=shapes, extra_samples={1: True}))
    out.append(build("n3_afreq_contigs", 3, 5, True, True, True, three, contigs=True))
    # both sides of the 64-lane stride, and two strides
    for n, lines, q, afreq, own in ((63, 5, True, True, True), (64, 6, False, False, False), (64, 5, True, True, False), (65, 8, True, True, True),
                                    (65, 5, False, True, False), (130, 6, True, True, True), (130, 5, True, False, False)):
        out.append(build("n%d_%s%s%s" % (n, "afreq" if afreq else "plain", "_q" if q else "", "_m" if own else ""), n, lines, q, afreq, own, one,
                         bare_info=True, extra_samples={n - 1: True, 3: True} if afreq else None))
    out.append(build("n3_forty_lines", 3, 40, True, True, True, one, bare_info=True))

    # every class the device leaves to the host's slow path, with bytes to write
    def slow(s, j, c):
        if j == 0 and s == 1:
            return _set(c, 5, "1743.00000000000011")            # a QUAL of 18 digits
        if j == 1 and s == 0:
            return _set(c, 5, " 12.5")                          # a QUAL float() strips
        if j == 2:                                              # eight ALTs
            return _set(c, 4, ",".join("<A%d>" % k for k in range(8))) if s < 0 else _gt(c, ("0/8", "3/7", "0/0")[s])
        if j == 3 and s == 2:
            return _gt(c, "0/0/0/0/0/0/0/0/1")                  # nine alleles
        if j == 4 and s == 1:
            return _gt(c, "+1/0")                               # a GT int() reads and the rule does not
        if j == 5 and s == 2:
            return c[:8]                                        # an input that is not the first, with eight columns
        if j == 6 and s < 0:
            return _set(c, 5, "1e3")
        if j == 7 and s == 0:
            return _set(c, 5, "inf")
        return c
    out.append(build("n3_slow_afreq_q", 3, 10, True, True, True, one, edit=slow, slow_lines=7))
    out.append(build("n3_slow_plain", 3, 10, False, False, True, one, edit=slow, slow_lines=4))           # (no GT is read without afreq)

    def slow65(s, j, c):
        if j == 1 and s == 64:
            return _set(c, 5, "0.30000000000000004")
        if j == 3 and s == 63:
            return _gt(c, "0/ 1")
        return c
    out.append(build("n65_slow_second_stride", 65, 5, True, True, True, one, edit=slow65, slow_lines=2, bare_info=True))

    # what ends the run
    short = build("n3_short_input", 3, 6, False, False, True, one)
    short["inputs"][1] = "".join(short["inputs"][1].splitlines(True)[:-2])
    short["error"] = dict(file=2, line=2 + 4 + 1, message=True)
    out.append(short)
    longer = build("n3_long_input", 3, 5, True, True, True, one)
    longer["inputs"][2] += longer["inputs"][2].splitlines(True)[-1]
    out.append(longer)
    out.append(build("n3_allele_beyond_alt", 3, 5, False, True, True, one, edit=lambda s, j, c: _gt(c, "0/2") if (s, j) == (1, 3) else c,
                     error=dict(file=2, line=2 + 3 + 1, message=False)))
    out.append(build("n2_qual_no_number", 2, 5, False, False, True, one, edit=lambda s, j, c: _set(c, 5, "high") if (s, j) == (1, 2) else c,
                     error=dict(file=2, line=2 + 2 + 1, message=False)))
    dot = build("n2_master_qual_dot_afreq", 2, 5, False, True, True, one, edit=lambda s, j, c: _set(c, 5, ".") if (s, j) == (-1, 1) else c)
    dot["error"] = dict(file=0, line=dot["master"].count("\n") - 5 + 1 + 1, message=False)
    out.append(dot)
    return out


def case_options(case):
    return dict(sum_quals=case["sum_quals"], afreq=case["afreq"])


def write_case(case, directory):
    """the case's files under `directory`: (master path or None, the inputs' paths)"""
    paths = []
    for k, text in enumerate(case["inputs"]):
        paths.append(os.path.join(directory, "in%03d.vcf" % k))
        with open(paths[-1], "w") as f:
            f.write(text)
    master = None
    if case["master"] is not None:
        master = os.path.join(directory, "master.vcf")
        with open(master, "w") as f:
            f.write(case["master"])
    return master, paths

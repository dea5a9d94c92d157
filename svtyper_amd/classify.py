"""`python -m svtyper_amd.classify`: the DEL and DUP lines of a cohort VCF tested for read-depth support.

    classify(vcf_in, gender, exclude=None, annotation=None, f_overlap=0.9, slope_threshold=1.0, rsquared_threshold=0.2,
             vcf_out=sys.stdout, engine="host", device=0, file_date=None, block_bytes=None, stats=None, keep_contigs=False)

The step that follows `svtyper_amd.paste --afreq` and a copy-number annotation in the reference's cohort workflow:
scripts/sv_classifier.py (`-i`, `-g`, `-e`, `-a`, `-f`, `-s`, `-r` mean what they mean there; the output is that script's, byte
for byte, but for the `##fileDate=` line, which is `file_date`, YYYYMMDD, default today).  The script is the specification, quirks
included: the header is rebuilt from the attributes of its ##INFO, ##ALT and ##FORMAT lines and everything else is dropped; a
line whose first INFO item "SVTYPE=" is neither DEL nor DUP goes through as it is; every other line is written again field by
field (QUAL '%0.2f', INFO and FORMAT in the header's order) when read depth supports it, and as two BND lines when not; on X and
Y the low-frequency test compares the chosen sex's 1/1 samples with its 0/1 samples, as the script's overwritten list has it.

Not in the reference: `-o`, `keep_contigs` (the input's ##contig lines stay, directly before the #CHROM line, so that the result
can be sorted by declared rank and written as BCF; as in svtyper_amd.paste), `engine` ("host": the native host twin; "device":
the HIP kernel of svtyper_amd/csrc/svt_vcf_classify_kernel.h; the same records, byte for byte, and the same text), and the output
options of the other programs (--bgzf / --bcf, --sort, --tabix / --csi, --deflate, --huffman).

Where the script dies with a traceback, ClassifyError names the file, the 1-based line and what was wrong (`reference`: the
script's exception); where it prints a message (a FORMAT key the header does not declare), the CLI prints the same message;
both end with status 1.  Two departures: the script ends with an AttributeError after its output is complete whenever `-e` is
absent, and here that run ends with status 0; a CN or AB that float() reads as nan or inf raises ClassifyError (the script goes
on with numpy's ordering of NaN).

The header and `-a` (the mobile-element annotation: a DEL that overlaps one becomes an MEI line before any depth test) run in
Python; the body goes through the native library in blocks of at most `block_bytes` of text (None: paste.BLOCK_BYTES[engine]):
the per-line records from either engine, the output text from one C++ writer.
"""
from __future__ import annotations

import argparse
import gzip
import sys
import time
from typing import Optional

import numpy as np

from . import native_reads as nr
from .cohort import (FORMAT_MESSAGE, _text, add_program_arguments, bad_line, begin_body, blocks, chrom_lines, finish_block, format_table,
                     header_attributes, info_table, parse_program_arguments, run_options, run_program, run_stats)
from .cohort import bytes_lines as _bytes_lines
from .cohort import open_source as _open

# the script's exception and what to say for each way a line can end the run (native_reads.CLASSIFY_BAD_*)
_KINDS = {nr.CLASSIFY_BAD_COLUMNS: ("IndexError", "fewer than eight columns"),
          nr.CLASSIFY_BAD_POS: ("ValueError", "a POS that is no integer: %(text)s"),
          nr.CLASSIFY_BAD_QUAL: ("ValueError", "a QUAL that is no number: %(text)s"),
          nr.CLASSIFY_BAD_FORMAT: (None, "a FORMAT key the header does not declare: %(text)s"),
          nr.CLASSIFY_BAD_KEY: ("KeyError", "%(where)s has no %(text)s"),
          nr.CLASSIFY_BAD_NUMBER: ("ValueError", "%(where)s has a CN or AB that is no number: %(text)s"),
          nr.CLASSIFY_BAD_NONFINITE: (None, "%(where)s has a CN or AB that is not finite: %(text)s"),
          nr.CLASSIFY_BAD_GENDER: ("KeyError", "%(where)s is not in the gender file")}
_VERBATIM = {nr.CLASSIFY_BAD_FORMAT: lambda text: FORMAT_MESSAGE % text}


class ClassifyError(Exception):
    """the input cannot be classified: `file` names it, `line` is the 1-based number of the line in the way; `reference`: the
    exception the script dies of there (None: it goes on, or prints `verbatim` and ends with status 1)"""

    def __init__(self, message, file=None, line=None, reference=None, verbatim=None):
        super().__init__(message)
        self.file, self.line, self.reference, self.verbatim = file, line, reference, verbatim


_bad = bad_line(ClassifyError, _KINDS, _VERBATIM)


def read_genders(source):
    """the gender file: {sample: the integer of its second column}"""
    name, f, own = _open(source)
    genders = {}
    try:
        for k, line in enumerate(_bytes_lines(f)):
            v = _text(line).rstrip().split("\t")
            try:
                genders[v[0]] = int(v[1])
            except (IndexError, ValueError) as e:
                raise ClassifyError("%s, line %d: a sample and its gender (male=1, female=2), tab-separated" % (name, k + 1), name, k + 1,
                                    type(e).__name__) from None
    finally:
        if own:
            f.close()
    return genders


def read_excluded(source):
    if source is None:
        return []
    name, f, own = _open(source)
    try:
        return [_text(line).rstrip() for line in _bytes_lines(f)]
    finally:
        if own:
            f.close()


def read_annotation(path):
    """the BED of annotated elements: {chrom: [[start, end, class, ...], ...]} in file order; lines of fewer than four columns are
    passed over.  The features are lists because the sweep merges them in place (annotation_class)"""
    elements = {}
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        for k, line in enumerate(f):
            v = _text(line).rstrip().split("\t")
            if len(v) < 4:
                continue
            try:
                v[1], v[2] = int(v[1]), int(v[2])
            except ValueError:
                raise ClassifyError("%s, line %d: a start or end that is no integer" % (path, k + 1), path, k + 1, "ValueError") from None
            elements.setdefault(v[0], []).append(v[1:])
    return elements


def _merged(features):
    """the features of one class, ordered by their END, a feature whose end reaches the next one's start taking that one's end.
    As the script has it, the merge changes the features themselves, so it lasts for the lines that follow"""
    ordered = sorted(features, key=lambda feature: feature[1])
    merged, current = [], ordered[0]
    for following in ordered[1:]:
        if current[1] >= following[0]:
            current[1] = following[1]
        else:
            merged.append(list(current))
            current = following
    merged.append(list(current))
    return merged


def _reciprocal(start, end, features):
    if end == start:
        return 0
    covered = sum(f[1] - f[0] for f in features)
    shared = 0
    for f in features:
        shared += float(min(end, f[1]) - max(start, f[0]))
    if covered == 0:
        return 0
    return min(shared / (end - start), shared / covered)


def annotation_class(chrom, start, end, elements, threshold):
    """the class of annotated elements whose merged features overlap [start, end) reciprocally by `threshold` at the least, the
    best such class, or None.  The sweep over the contig's features ends at the first that starts at or beyond `end`"""
    if chrom not in elements:
        return None
    by_class = {}
    for feature in elements[chrom]:
        if not feature[0] < end:
            break
        if feature[1] > start:
            by_class.setdefault(feature[2], []).append(feature)
    best, best_class = 0, ""
    for name in by_class:
        fraction = _reciprocal(start, end, _merged(by_class[name]))
        if fraction > best:
            best, best_class = fraction, name
    return best_class if best >= threshold else None


class _Variant:
    """the script's Variant of one line, for `-a`: what the annotation reads (CHROM, POS, END) and the MEI line it may write.
    The native writer holds the same rules for every other line (svt_vcf_classify.h: parse_variant, var_string)"""

    def __init__(self, line, samples, infos, formats, name, number):
        v = line.rstrip().split("\t")
        if len(v) < 8:
            raise _bad(name, number, nr.CLASSIFY_BAD_COLUMNS)
        self.first = v[:7]
        try:
            self.pos = int(v[1])
        except ValueError:
            raise _bad(name, number, nr.CLASSIFY_BAD_POS, v[1]) from None
        try:
            self.qual = 0 if v[5] == "." else float(v[5])
        except ValueError:
            raise _bad(name, number, nr.CLASSIFY_BAD_QUAL, v[5]) from None
        if len(v) < 9:
            v.append("GT")
        ids = [f[0] for f in formats]
        self.active, self.genotypes = set(), []
        for k in range(len(samples)):
            fields = {}
            if 9 + k < len(v):
                column = v[9 + k].split(":")
                fields["GT"] = column[0]
                for key, value in zip(v[8].split(":"), column):
                    if key not in ids:
                        raise _bad(name, number, nr.CLASSIFY_BAD_FORMAT, key)
                    fields[key] = value
            else:
                fields["GT"] = "./."
            self.active.update(fields)
            self.genotypes.append(fields)
        self.info = {}
        for item in v[7].split(";"):
            parts = item.split("=")
            self.info[parts[0]] = parts[1] if len(parts) > 1 else True
        self.infos, self.ids = infos, ids

    def text(self, alt):
        info = ";".join(i if t == "Flag" else "%s=%s" % (i, self.info[i]) for i, _, t, _ in self.infos if i in self.info)
        active = [i for i in self.ids if i in self.active]
        columns = [":".join(g.get(i, ".") for i in active) for g in self.genotypes]
        return "\t".join([self.first[0], str(self.pos), self.first[2], self.first[3], alt, "%0.2f" % self.qual, self.first[6], info,
                          ":".join(active), "\t".join(columns)]) + "\n"


def _first_svtype(line: bytes):
    columns = line.rstrip().split(b"\t")
    if len(columns) < 8:
        return None
    for item in columns[7].split(b";"):
        if item.startswith(b"SVTYPE="):
            return item.split(b"=")[1]
    return None


def _annotate(block, elements, f_overlap, samples, infos, formats, name, done):
    """`-a` over the lines of a block, in order, before any depth test: (skip, mei, pending).  skip[j] = 1 and mei[j] the text
    for a line that becomes an MEI.  A line the script dies on while it parses or annotates it: `pending` is its ClassifyError
    and skip ends in front of it, so that the lines in front are tested and written first (an error there comes first)"""
    skip, mei = np.zeros(len(block), np.uint8), {}
    for j, data in enumerate(block):
        first = _first_svtype(data)
        # (the script parses every DEL and DUP line and annotates by the LAST SVTYPE item: a line that starts as a DUP too)
        if first != b"DEL" and not (first == b"DUP" and data.count(b"SVTYPE") > 1):
            continue
        number = done + j + 1
        try:
            var = _Variant(_text(data), samples, infos, formats, name, number)
            if var.info.get("SVTYPE") != "DEL" or var.first[0] not in elements:
                continue
            try:                                    # (END is looked at only where the BED holds the contig)
                end = int(var.info["END"])
            except KeyError:
                raise _bad(name, number, nr.CLASSIFY_BAD_KEY, "END") from None
            except ValueError:
                raise ClassifyError("%s, line %d: an END that is no integer" % (name, number), name, number, "ValueError") from None
            found = annotation_class(var.first[0], var.pos, end, elements, f_overlap)
            if found is None:
                continue
            if not (found.startswith("SINE") or found.startswith("LINE")):
                parts = found.split("|")
                if len(parts) < 3:
                    raise ClassifyError("%s, line %d: the annotated class %s has no third '|' field" % (name, number, found), name, number,
                                        "IndexError")
                if parts[2].startswith("SVA"):
                    found = "ME:" + found
            else:
                found = "ME:" + found
        except ClassifyError as e:
            return skip[:j], mei, e
        var.info["SVTYPE"] = "MEI"
        skip[j] = 1
        mei[j] = var.text("<DEL:%s>" % found)
    return skip, mei, None


def classify(vcf_in, gender, exclude=None, annotation=None, f_overlap=0.9, slope_threshold=1.0, rsquared_threshold=0.2, vcf_out=sys.stdout,
             engine="host", device=0, file_date=None, block_bytes=None, stats: Optional[dict] = None, keep_contigs=False):
    """`vcf_in`, `gender`, `exclude`: paths (a path ending in .gz is read through gzip) or open files; `annotation`: the path of a BED
    (or BED.gz) of annotated elements.  `vcf_out`: any text sink the drivers accept; it is not closed.  `stats`, a dict, receives
    lines, blocks, host_lines (the lines the host's plain C++ decided), near_lines (the lines whose r2 or slope lies within 1e-9 of
    its threshold), results (the per-line records of every block, native_reads.CLASSIFY_LINE) and, for engine="device", times (the
    sums of vcf_classify_last_times)."""
    block_bytes = run_options(engine, block_bytes)
    stats = run_stats(stats, lines=0, blocks=0, host_lines=0, near_lines=0, results=[], times={})
    genders, excluded = read_genders(gender), set(read_excluded(exclude))
    elements = read_annotation(annotation) if annotation is not None else None
    name, f, own = _open(vcf_in, engine=engine, device=device)
    try:
        _run(name, _bytes_lines(f), genders, excluded, elements, f_overlap, slope_threshold, rsquared_threshold, vcf_out,
             device if engine == "device" else None, file_date or time.strftime("%Y%m%d"), block_bytes, stats, keep_contigs)
    finally:
        if own:
            f.close()


def header_tables(header):
    """what the output header is made of, from the input's header lines: (fileformat, reference, the INFO, ALT and FORMAT tables, the
    samples of the last line that begins with one '#' alone: none without such a line)"""
    file_format, reference, _filters, infos, alts, formats = header_attributes([h.rstrip("\n") for h in header if h.startswith("##")], ClassifyError)
    return file_format, reference, infos, alts, formats, ([""] + chrom_lines(header))[-1].rstrip().split("\t")[9:]


def _run(name, lines, genders, excluded, elements, f_overlap, slope_threshold, rsquared_threshold, vcf_out, device, file_date, block_bytes, stats,
         keep_contigs):
    body = begin_body(name, lines, vcf_out, file_date, keep_contigs, header_tables, None, with_format=True)
    if body is None:
        return
    done, first, samples, infos, formats = body                 # done: lines of the file in front of the block
    info_bytes, format_bytes = info_table(infos), format_table(formats)
    male = np.array([1 if genders.get(s) == 1 else nr.CLASSIFY_NO_GENDER if s not in genders else 0 for s in samples], np.uint8)
    female = np.array([1 if genders.get(s) == 2 else nr.CLASSIFY_NO_GENDER if s not in genders else 0 for s in samples], np.uint8)
    skipped = np.array([s in excluded for s in samples], np.uint8)
    for block in blocks(first, lines, block_bytes):
        bare = not block[-1].endswith(b"\n")        # (the file's last line: rewritten lines end in a newline all the same)
        text = b"".join(block) + (b"\n" if bare else b"")
        skip, mei, pending = None, {}, None
        if elements is not None:                    # (a line the annotation dies on ends the block: the lines in front come first)
            skip, mei, pending = _annotate(block, elements, f_overlap, samples, infos, formats, name, done)
            if pending is not None:
                block = block[:int(skip.shape[0])]
                if not block:
                    raise pending
                bare = False
                text = b"".join(block)
        records = nr.vcf_classify(text, male, female, skipped, format_bytes, slope_threshold, rsquared_threshold, skip, device)

        def edit(out, out_off, written, whole):     # (called once, by finish_block below)
            if not written["bad_line"] and bare and whole == len(block) and records[0][-1]["route"] == nr.CLASSIFY_VERBATIM:
                out = out[:-1]
            pieces, at = [], 0                      # `-a`: an MEI's text stands in front of its line's (empty) output
            for j in sorted(k for k in mei if k < whole):
                pieces += [out[at:int(out_off[j])], mei[j].encode("utf-8", "surrogateescape")]
                at = int(out_off[j])
            return b"".join(pieces) + out[at:]

        finish_block(name, done, block, text, samples, records,
                     lambda kept, results: nr.vcf_classify_write(kept, len(samples), info_bytes, format_bytes, results),
                     nr.vcf_classify_last_times if device is not None else None, _bad, vcf_out, stats, edit)
        if pending is not None:
            raise pending
        done += len(block)


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-classify", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-classify\ndescription: classify structural variants by read-depth support"))
    p.add_argument("-i", "--input", metavar="VCF", dest="vcf_in", type=str, default=None, help="VCF input, .gz through gzip [stdin]")
    p.add_argument("-g", "--gender", metavar="FILE", required=True, help="tab delimited file of sample genders (male=1, female=2)\nex: SAMPLE_A\t2")
    p.add_argument("-e", "--exclude", metavar="FILE", default=None, help="list of samples to exclude from classification algorithms")
    p.add_argument("-a", "--annotation", metavar="BED", default=None, help="BED file of annotated elements")
    p.add_argument("-f", "--fraction", metavar="FLOAT", dest="f_overlap", type=float, default=0.9,
                   help="fraction of reciprocal overlap to apply annotation to variant [0.9]")
    p.add_argument("-s", "--slope_threshold", metavar="FLOAT", type=float, default=1.0,
                   help="minimum slope absolute value of regression line to classify as DEL or DUP [1.0]")
    p.add_argument("-r", "--rsquared_threshold", metavar="FLOAT", type=float, default=0.2,
                   help="minimum R^2 correlation value of regression line to classify as DEL or DUP [0.2]")
    add_program_arguments(p, "where the lines are tested: the native host code or the GPU (same output bytes) [host]")
    return parse_program_arguments(p, argv, "vcf_in")


def main(argv=None):
    args = get_args(argv)
    call = dict(exclude=args.exclude, annotation=args.annotation, f_overlap=args.f_overlap, slope_threshold=args.slope_threshold,
                rsquared_threshold=args.rsquared_threshold, engine=args.engine, device=args.device, keep_contigs=args.keep_contigs)
    vcf_in = args.vcf_in if args.vcf_in is not None else sys.stdin.buffer
    return run_program(args, ClassifyError, lambda out: classify(vcf_in, args.gender, vcf_out=out, **call))


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

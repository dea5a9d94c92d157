"""What the cohort programs share (svtyper_amd.paste, svtyper_amd.classify, svtyper_amd.update_info, svtyper_amd.group_multiline,
svtyper_amd.modify_header, svtyper_amd.bcf_in); none of them imports another.

The input: how it is opened (open_source), how its header is read (read_header, chrom_lines) and what the Vcf class of the
reference's scripts reads off it (header_attributes, add_attributes) and writes again (declared_lines, header_text).  The native
calls: their INFO and FORMAT tables (info_table, format_table), how much text a block holds (BLOCK_BYTES, blocks) and what becomes
of a block's records (finish_block).  A program's frame: the checks on engine and block_bytes (run_options) and stats (run_stats), the head of a run
up to the first body line (begin_body), the exception of a line that ends the run (bad_line) and the command line: the options
every program has (add_program_arguments, parse_program_arguments) and the output with its error tail (run_program)."""
from __future__ import annotations

import argparse
import gzip
import re
import sys
from typing import Iterable, Iterator, List, Optional, Tuple

GZIP_MAGIC = b"\x1f\x8b"
# a block's lines are a launch's wavefronts, so the device wants many; the host twin is fastest with blocks its caches hold
BLOCK_BYTES = {"host": 8 << 20, "device": 64 << 20}
# what the scripts print where they end without a traceback
FORMAT_MESSAGE = '\nError: invalid FORMAT field, "%s"\n'
COLUMNS_MESSAGE = "\nError: VCF file must have at least 8 columns\n"
_ATTRIBUTES = re.compile(r'(?:[^,"]|"[^"]*")+')         # the attributes of a header line's <...>: commas inside quotes do not split


def open_source(source, sniff=False, engine="host", device=0):
    """(name, binary or text file, whether it is ours to close) of a path or an open file.  A path ending in .gz is read through
    gzip; `sniff`: so is whatever begins with the two bytes of a gzip member (an open file must be able to peek for that).  A BCF
    is read as its VCF text (bcf_in.open_text, decoded by `engine` on `device`): a path ending in .bcf, and with `sniff` whatever
    is BGZF whose payload begins with the BCF magic"""
    if isinstance(source, (str, bytes)):
        name = source if isinstance(source, str) else source.decode()
        zipped = name.endswith(".gz")
        bcf = name.endswith(".bcf")
        if sniff and not bcf:
            with open(name, "rb") as f:
                zipped = zipped or f.read(2) == GZIP_MAGIC
            bcf = zipped and _is_bcf(name)
        if bcf:
            return name, _bcf_text(name, engine, device), True
        return name, (gzip.open(name, "rb") if zipped else open(name, "rb")), True
    name = str(getattr(source, "name", source))
    if sniff and hasattr(source, "peek") and source.peek(2)[:2] == GZIP_MAGIC:
        if _is_bcf(source):
            return name, _bcf_text(source, engine, device), True
        return name, gzip.GzipFile(fileobj=source, mode="rb"), False
    return name, source, False


def _is_bcf(source):
    from . import bcf_in
    return bcf_in.is_bcf(source)


def _bcf_text(source, engine, device):
    from . import bcf_in
    return bcf_in.open_text(source, engine=engine, device=device)


def bytes_lines(f) -> Iterator[bytes]:
    for line in f:
        yield line.encode("utf-8", "surrogateescape") if isinstance(line, str) else line


def read_header(lines: Iterator[bytes]) -> Tuple[List[str], Optional[bytes]]:
    """(the lines in front of the first that does not begin with '#', that line or None)"""
    header = []
    for line in lines:
        if line[:1] != b"#":
            return header, line
        header.append(line.decode("utf-8", "surrogateescape"))
    return header, None


def chrom_lines(header: List[str]) -> List[str]:
    """the header's lines that begin with one '#' alone: the last of them names the samples"""
    return [h for h in header if h[1:2] != "#"]


def header_text(file_format, file_date, reference, declared: List[str], header: List[str], samples: List[str], keep_contigs, with_format=True):
    """the scripts' get_header: fileformat, fileDate, reference, the declared lines, the input's ##contig lines where they are
    kept, and the #CHROM line (`with_format`: its FORMAT column and the samples)"""
    columns = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] + (["FORMAT"] + samples if with_format else [])
    return "\n".join(["##fileformat=" + file_format, "##fileDate=" + file_date, "##reference=" + reference] + declared
                     + ([h.rstrip("\n") for h in header if h.startswith("##contig")] if keep_contigs else []) + ["\t".join(columns)]) + "\n"


def _text(data: bytes) -> str:
    return data.decode("utf-8", "surrogateescape")


def _attributes(line: str, end):
    inside = line[line.find("<") + 1:end(line)]
    return [a.split("=")[1] for a in _ATTRIBUTES.findall(inside)]


def _unquoted(desc: str) -> str:
    return desc[1:-1] if desc.startswith('"') and desc.endswith('"') else desc


def add_attributes(table, values, width, error):
    """one header line's attributes into its table, the first line of an ID winning"""
    if len(values) != width:
        raise error("a header line with %d attributes where %d are read: %s" % (len(values), width, ",".join(values)))
    if values[0] not in [row[0] for row in table]:
        table.append(tuple(values))


def header_attributes(header_lines: List[str], error):
    """What the Vcf class of the reference's scripts (vcf_allele_freq.py, sv_classifier.py) reads off a header (`header_lines`
    without their newlines): (fileformat, reference, FILTER, INFO, ALT, FORMAT tables), GT the first FORMAT; `error`: the
    exception of a line whose attributes cannot be read"""
    file_format, reference = "VCFv4.2", ""
    filters, infos, alts, formats = [], [], [], [("GT", "1", "String", "Genotype")]

    def add(table, values, width):
        add_attributes(table, values, width, error)

    for bare in header_lines:
        line = bare + "\n"
        key = line.split("=")[0]
        try:
            if key == "##fileformat":
                file_format = line.rstrip().split("=")[1]
            elif key == "##reference":
                reference = line.rstrip().split("=")[1]
            elif key == "##INFO":
                add(infos, _attributes(line, lambda t: t.find(">")), 4)
            elif key == "##ALT":
                add(alts, _attributes(line, lambda t: t.find(">")), 2)
            elif key == "##FORMAT":
                add(formats, _attributes(line, lambda t: t.find(">")), 4)
            elif key == "##FILTER":
                add(filters, _attributes(line, lambda t: -2), 2)
        except IndexError:
            raise error("a header line whose attributes are not key=value: %s" % bare) from None
    return file_format, reference, filters, infos, alts, formats


def declared_lines(infos, alts, formats) -> List[str]:
    """the ##INFO, ##ALT and ##FORMAT lines rebuilt from their attributes"""
    out = ['##INFO=<ID=%s,Number=%s,Type=%s,Description="%s">' % (i, n, t, _unquoted(d)) for i, n, t, d in infos]
    out += ['##ALT=<ID=%s,Description="%s">' % (i, _unquoted(d)) for i, d in alts]
    out += ['##FORMAT=<ID=%s,Number=%s,Type=%s,Description="%s">' % (i, n, t, _unquoted(d)) for i, n, t, d in formats]
    return out


def info_table(infos) -> bytes:
    """the INFO table of the native calls: "V<id>\\n" per id in the header's order, "F<id>\\n" for a Flag"""
    return "".join(("F" if t == "Flag" else "V") + i + "\n" for i, _, t, _ in infos).encode("utf-8", "surrogateescape")


def format_table(formats) -> bytes:
    """the FORMAT table of the native calls: "<id>\\n" per id in the header's order, GT first"""
    return "".join(i + "\n" for i, _, _, _ in formats).encode("utf-8", "surrogateescape")


def blocks(first: bytes, lines: Iterable[bytes], block_bytes: int) -> Iterator[List[bytes]]:
    """the body from `first` on in lists of lines of at most `block_bytes` together, a line at the least"""
    block, size = [first], len(first)
    for line in lines:
        if size + len(line) <= block_bytes:
            block.append(line)
            size += len(line)
            continue
        yield block
        block, size = [line], len(line)
    yield block


def finish_block(name, done, block, text, samples, records, write, last_times, bad, vcf_out, stats, edit=None):
    """What follows a block's records in both programs: the lines in front of the one the script dies on are counted, joined again
    and written (write(text, results) -> out, out_off, report; edit(out, out_off, report, whole) -> out may change the text), the
    stats and the device's times are folded in, and the writer's report, then the records', is raised through bad(name, line, kind,
    text, sample).  `records`: (results, report) of the native call over `text`; `done`: the file's lines in front of the block"""
    results, info = records
    whole = info["bad_line"] - 1 if info["bad_line"] else len(block)
    if whole < len(block):
        text = b"".join(block[:whole])
    out, out_off, written = write(text, results[:whole])
    if written["bad_line"]:
        whole = written["bad_line"] - 1
    if edit is not None:
        out = edit(out, out_off, written, whole)
    vcf_out.write(out.decode("utf-8", "surrogateescape"))
    stats["lines"] += whole
    stats["blocks"] += 1
    for key in ("host_lines", "near_lines"):
        if key in info:
            stats[key] += info[key]
    stats["results"].append(results)
    if last_times is not None:
        for key, value in last_times().items():
            stats["times"][key] = stats["times"].get(key, 0.0) + value
    for report in (written, info):
        if report["bad_line"]:
            sample = samples[report["bad_sample"]] if report["bad_sample"] < len(samples) else None
            raise bad(name, done + whole + 1, report["bad_kind"], report["bad_text"], sample)


# ------------------------------------------------------------------------------------------ a program's frame
def run_options(engine, block_bytes=None):
    """the block_bytes of a program's call (None: BLOCK_BYTES[engine]), or the ValueError of an engine or a block_bytes that is none"""
    if engine not in ("host", "device"):
        raise ValueError("engine is 'host' or 'device'")
    if block_bytes is None:
        block_bytes = BLOCK_BYTES[engine]
    if block_bytes < 1:
        raise ValueError("block_bytes is at least 1")
    return block_bytes


def run_stats(stats, **counters):
    """the caller's `stats` (None: a new dict) with `counters` set"""
    if stats is None:
        stats = {}
    stats.update(counters)
    return stats


def begin_body(name, lines, vcf_out, file_date, keep_contigs, header_tables, error, with_format=None):
    """The head of a run: the header is read and, where a body line follows, written again from header_tables(header) ->
    (fileformat, reference, INFO, ALT and FORMAT tables, samples).  None where there is no body line (nothing is written), else
    (the lines in front of the body, the first body line, the samples, the INFO table and the FORMAT table of the header).
    `error`: the program's exception of a body line with no #CHROM line in front of it (None: the script goes on there, with the
    samples its header_tables gives).  `with_format`: whether the #CHROM line has FORMAT and the samples (None: where there are
    samples)"""
    header, first = read_header(lines)
    if first is None:                               # (the header is written when the first body line is met)
        return None
    done = len(header)                              # lines of the file in front of the body
    if error is not None and not chrom_lines(header):       # (the script's sample list is never bound)
        raise error("%s, line %d: a body line and no #CHROM line in front of it" % (name, done + 1), name, done + 1, reference="UnboundLocalError")
    file_format, reference, infos, alts, formats, samples = header_tables(header)
    vcf_out.write(header_text(file_format, file_date, reference, declared_lines(infos, alts, formats), header, samples, keep_contigs,
                              with_format=bool(samples) if with_format is None else with_format))
    return done, first, samples, infos, formats


def bad_line(error, kinds, verbatim, fields=()):
    """bad(name, line, kind, text="", sample=None) -> the program's `error` of a line that ends the run.  kinds[kind]: (the script's
    exception, what to say); verbatim[kind](text): what the script prints instead, where it prints; `fields`: which of sample and
    token the exception takes beside file, line, reference and verbatim"""
    def bad(name, line, kind, text="", sample=None):
        reference, what = kinds[kind]
        where = "the line" if sample is None else "sample %s" % sample
        more = {key: value for key, value in (("sample", sample), ("token", text or None)) if key in fields}
        return error("%s, line %d: %s" % (name, line, what % dict(text=text, where=where)), file=name, line=line, reference=reference,
                     verbatim=verbatim[kind](text) if kind in verbatim else None, **more)
    return bad


def add_program_arguments(p, engine_help, keep_contigs_help="keep the input's ##contig lines, directly before the #CHROM line"):
    """the options every cohort program has, behind its own: --keep-contigs (None: the program has none), -o, --engine, --device and
    the output options of the drivers"""
    from .driver import add_output_arguments
    if keep_contigs_help is not None:
        p.add_argument("--keep-contigs", dest="keep_contigs", action="store_true", help=keep_contigs_help)
    p.add_argument("-o", "--output_vcf", metavar="FILE", type=argparse.FileType("w"), default=sys.stdout,
                   help="output VCF to write (default: stdout)")
    p.add_argument("--engine", choices=("host", "device"), default="host", help=engine_help)
    p.add_argument("--device", metavar="INT", type=int, default=0, help="the GPU of --engine device and --deflate device [0]")
    add_output_arguments(p)


def parse_program_arguments(p, argv, stdin_for=None):
    """the arguments, the output options checked.  `stdin_for`: the dest of an input that defaults to stdin; where it is not given
    and stdin is a terminal the help is printed and the program ends with status 1"""
    from .driver import check_output_arguments
    args = p.parse_args(argv)
    check_output_arguments(p, args, args.output_vcf)
    if stdin_for is not None and getattr(args, stdin_for) is None and sys.stdin.isatty():
        p.print_help()
        sys.exit(1)
    return args


def run_program(args, error, run) -> int:
    """run(vcf_out) with the sink the output options ask for; the program's status: 1 where `error` is raised, with its `verbatim` or
    "Error: ..." on stderr"""
    from .driver import _bgzf_text
    try:
        if args.bgzf or args.bcf:
            with _bgzf_text(args.output_vcf, args.deflate, args.device, args.huffman, args) as out:
                run(out)
        else:
            run(args.output_vcf)
            args.output_vcf.flush()
    except error as e:
        sys.stderr.write(e.verbatim if e.verbatim is not None else "Error: %s\n" % e)
        return 1
    return 0

"""`python -m svtyper_amd.paste`: per-sample VCFs joined into one cohort VCF, with AF and NSAMP.

    paste(vcf_list, master=None, sum_quals=False, afreq=False, safe=False, keep_contigs=False, vcf_out=sys.stdout,
          engine="host", device=0, file_date=None, block_bytes=None)

The two steps that follow one `svtyper-sso` per sample in the reference's workflow: scripts/vcf_paste.py (`-f`, `-m`, `-q` mean
what they mean there; without `afreq` the output is that script's, byte for byte) and, with `afreq`, scripts/vcf_allele_freq.py
behind it (the output of the pipe of both, byte for byte, but for the `##fileDate=` line, which is `file_date`, YYYYMMDD, default
today).  The scripts are the specification, quirks included: lines are joined by number alone, FORMAT is the first input's, the
`-q` QUAL is Python 2's str(float), vcf_allele_freq.py rebuilds the header (and drops its ##contig lines) and INFO.

Not in the reference: `safe` (every input's CHROM, POS and ID must equal the master's: the check the reference has commented
out), `keep_contigs` (with `afreq`: the master's ##contig lines stay, directly before the #CHROM line, so that the result can be
sorted by declared rank and written as BCF), `engine` ("host": the native host twin; "device": the HIP kernels of
svtyper_amd/csrc/svt_vcf_paste_kernel.h; the same bytes), and the output options of the other two programs (--bgzf / --bcf,
--sort, --tabix / --csi, --deflate, --huffman).

Where a script dies with a traceback, PasteError names the file, the 1-based line and, for `safe`, the field; where it prints a
message (an input shorter than the master), the CLI prints the same message; both end with status 1.  One case is not followed:
a master whose header has no #CHROM line makes vcf_allele_freq.py print nothing at all, and so does `afreq` here, without reading
the body.

The header runs once, in Python; the body goes through the native library in blocks of at most `block_bytes` of text (at
least one line of every file; None: cohort.BLOCK_BYTES[engine]).
"""
from __future__ import annotations

import argparse
import gzip
import itertools
import sys
import time
from typing import List, Optional

import numpy as np

from . import native_reads as nr
from .cohort import (_text, _unquoted, add_attributes, add_program_arguments, declared_lines, header_attributes, info_table, open_source,
                     parse_program_arguments, run_options, run_program, run_stats)

LENGTH_MESSAGE = "\nError: VCF files differ in length\n"
FIELDS = ("CHROM", "POS", "ID")
_KINDS = {nr.PASTE_BAD_QUAL: "a QUAL that is no number", nr.PASTE_BAD_COLUMNS: "too few columns",
          nr.PASTE_BAD_GT: "a GT that is no list of allele numbers", nr.PASTE_BAD_ALLELE: "an allele number beyond the ALT count",
          nr.PASTE_BAD_POS: "a POS that is no integer"}


class PasteError(Exception):
    """the inputs cannot be joined: `file` names the one in the way, `line` is the 1-based number of its line, `field` the column
    `safe` found to differ; `verbatim`: the message the reference prints for this, where it prints one"""

    def __init__(self, message, file=None, line=None, field=None, verbatim=None):
        super().__init__(message)
        self.file, self.line, self.field, self.verbatim = file, line, field, verbatim


class _Lines:
    """the lines of one file, read ahead and handed back where a block has no room for them"""

    def __init__(self, source, engine="host", device=0):
        if isinstance(source, (str, bytes)):
            self.name = source if isinstance(source, str) else source.decode()
            if self.name.endswith(".bcf"):          # (by its suffix, as .gz is: cohort.open_source decodes it)
                self.f = open_source(self.name, engine=engine, device=device)[1]
            else:
                self.f = gzip.open(self.name, "rb") if self.name.endswith(".gz") else open(self.name, "rb")
        else:
            self.name = str(getattr(source, "name", source))
            self.f = source
        self.pending: List[bytes] = []
        self.taken = 0                              # lines handed out and not handed back

    def readline(self) -> bytes:
        line = self.pending.pop(0) if self.pending else self.f.readline()
        if isinstance(line, str):
            line = line.encode("utf-8", "surrogateescape")
        self.taken += bool(line)
        return line

    def take(self, n: int) -> List[bytes]:
        lines = self.pending[:n]
        del self.pending[:n]
        if len(lines) < n:
            more = list(itertools.islice(self.f, n - len(lines)))
            if more and isinstance(more[0], str):
                more = [line.encode("utf-8", "surrogateescape") for line in more]
            lines += more
        self.taken += len(lines)
        return lines

    def unread(self, lines: List[bytes]) -> None:
        self.pending[:0] = lines
        self.taken -= len(lines)

    def close(self) -> None:
        self.f.close()


def afreq_header(header_lines: List[str], chrom_line: str, file_date: str, keep_contigs: bool):
    """vcf_allele_freq.py's header for the pasted header (`header_lines` without their newlines): (text, INFO table of the native
    call).  fileformat, fileDate, reference, then the FILTER, INFO, ALT and FORMAT lines rebuilt from their attributes, GT the
    first FORMAT, AF and NSAMP behind the declared INFOs; everything else is dropped, ##contig too unless `keep_contigs`"""
    file_format, reference, filters, infos, alts, formats = header_attributes(header_lines, PasteError)
    add_attributes(infos, ["AF", "A", "Float", "Allele Frequency, for each ALT allele, in the same order as listed"], 4, PasteError)
    add_attributes(infos, ["NSAMP", "1", "Integer", "Number of samples with non-reference genotypes"], 4, PasteError)
    out = ["##fileformat=" + file_format, "##fileDate=" + file_date, "##reference=" + reference]
    out += ['##FILTER=<ID=%s,Description="%s">' % (i, _unquoted(d)) for i, d in filters]
    out += declared_lines(infos, alts, formats)
    if keep_contigs:
        out += [line for line in header_lines if line.startswith("##contig")]
    out.append("\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"]))
    text = "\n".join(out) + "\t" + "\t".join(chrom_line.rstrip().split("\t")[8:]) + "\n"
    return text, info_table(infos)


def paste(vcf_list, master=None, sum_quals=False, afreq=False, safe=False, keep_contigs=False, vcf_out=sys.stdout, engine="host",
          device=0, file_date=None, block_bytes=None, stats: Optional[dict] = None, layout="default"):
    """`vcf_list`: the inputs' paths (or binary files) in order; `master`: a path or a binary file, None for a second handle on
    the first input.  `vcf_out`: any text sink the drivers accept (a file, bgzf_out.open_text(...), bcf_out.open_bcf(...)); it is
    not closed.  `stats`, a dict, receives lines, blocks, host_lines (the lines the host's slow path wrote), results (the per-line
    records of every block, native_reads.PASTE_LINE) and, for engine="device", times (the sums of vcf_paste_last_times).
    `layout`: how the device's write kernel spreads its lanes over the sample parts (native_reads.PASTE_LAYOUTS)."""
    block_bytes = run_options(engine, block_bytes)
    vcf_list = list(vcf_list)
    if not vcf_list:
        raise PasteError("no input: the list of VCF files is empty")
    inputs = [_Lines(v, engine, device) for v in vcf_list]
    files = [_Lines(master if master is not None else inputs[0].name, engine, device)] + inputs
    stats = run_stats(stats, lines=0, blocks=0, host_lines=0, results=[], times={})
    try:
        _run(files, sum_quals, afreq, safe, keep_contigs, vcf_out, engine, device, file_date, block_bytes, stats, layout)
    finally:
        for f in files:
            if f.f is not master and f.f not in vcf_list:       # (what was handed in open stays the caller's)
                f.close()


def _run(files, sum_quals, afreq, safe, keep_contigs, vcf_out, engine, device, file_date, block_bytes, stats, layout):
    master, inputs = files[0], files[1:]
    # the header: the master's ## lines right-stripped; #CHROM is its first nine fields and every input's from the tenth on
    header = []
    while True:
        chrom_line = master.readline()
        if not chrom_line or chrom_line[:2] != b"##":
            break
        header.append(chrom_line.rstrip())
    columns = chrom_line.rstrip().split(b"\t", 9)[:9]
    for f in inputs:
        while True:
            line = f.readline()
            if not line:
                break
            if line[:2] == b"##":
                continue
            if line[:1] == b"#":
                columns += line.rstrip().split(b"\t", 9)[9:]
                break
    pasted_chrom = b"\t".join(columns)
    info_table = b""
    if afreq:
        if not pasted_chrom.startswith(b"#CHROM"):
            return
        text, info_table = afreq_header([_text(h) for h in header], _text(pasted_chrom), file_date or time.strftime("%Y%m%d"), keep_contigs)
        vcf_out.write(text)
    else:
        vcf_out.write(_text(b"".join(h + b"\n" for h in header) + pasted_chrom + b"\n"))
    first_body = [f.taken for f in files]           # the lines of each file in front of its body
    flags = (nr.PASTE_SUM_QUALS if sum_quals else 0) | (nr.PASTE_AFREQ if afreq else 0) | (nr.PASTE_SAFE if safe else 0)
    done = 0                                        # body lines written
    n = len(inputs)
    while True:
        first = master.take(1)
        if not first:
            return
        row = [first] + [f.take(1) for f in inputs]
        rows = max(1, block_bytes // max(sum(len(r[0]) for r in row if r), 1))
        block = [r + (f.take(rows - 1) if r else []) for r, f in zip(row, files)]
        have = min(len(b) for b in block)
        short = have < len(block[0])                # an input ends before the master does
        keep = 0                                    # no more lines than block_bytes hold, but one at the least
        if have:
            sizes = np.cumsum(np.sum([np.fromiter(map(len, b[:have]), np.int64, have) for b in block], axis=0))
            keep = max(int(np.searchsorted(sizes, block_bytes - len(block), side="right")), 1)       # (a newline a file's last line may lack)
        if keep < have:
            short = False
        for f, b in zip(files, block):
            f.unread(b[keep:])
        if keep:
            text = b"".join(data if data.endswith(b"\n") else data + b"\n" for data in (b"".join(b[:keep]) for b in block))
            out, results, info = nr.vcf_paste(text, [k * keep for k in range(n + 1)], n, keep, flags, info_table,
                                              device=device if engine == "device" else None, layout=layout)
            if info["bad_line"]:
                f = files[info["bad_file"]]
                line = first_body[info["bad_file"]] + done + info["bad_line"]
                if info["bad_kind"] == nr.PASTE_BAD_UNSAFE:
                    field = FIELDS[info["bad_field"]]
                    raise PasteError("%s, line %d: %s differs from the master's (%s)" % (f.name, line, field, master.name), f.name, line, field)
                raise PasteError("%s, line %d: %s" % (f.name, line, _KINDS[info["bad_kind"]]), f.name, line)
            vcf_out.write(_text(out))
            done += keep
            stats["lines"] += keep
            stats["blocks"] += 1
            stats["host_lines"] += info["host_lines"]
            stats["results"].append(results)
            if engine == "device":
                for name, value in nr.vcf_paste_last_times().items():
                    stats["times"][name] = stats["times"].get(name, 0.0) + value
        if short:
            k = min(range(1, n + 1), key=lambda k: len(block[k]))
            raise PasteError("%s, line %d: the file ends before the master does" % (files[k].name, first_body[k] + done + 1), files[k].name,
                             first_body[k] + done + 1, verbatim=LENGTH_MESSAGE)


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-paste", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-paste\ndescription: Paste VCFs from multiple samples; optionally add allele frequency information"))
    p.add_argument("-m", "--master", metavar="FILE", type=str, default=None,
                   help="VCF file to set first 8 columns of variant info [first file in vcf_list]")
    p.add_argument("-q", "--sum_quals", action="store_true", help="Sum QUAL scores of input VCFs as output QUAL score")
    p.add_argument("-f", "--vcf_list", metavar="FILE", required=True, help="Line-delimited list of VCF files to paste")
    p.add_argument("--afreq", action="store_true", help="add AF and NSAMP to INFO, as vcf_allele_freq.py does to the pasted VCF")
    p.add_argument("--safe", action="store_true", help="check that CHROM, POS and ID of every input's lines match the master's")
    add_program_arguments(p, "where the lines are joined: the native host code or the GPU (same output bytes) [host]",
                          "with --afreq: keep the master's ##contig lines, directly before the #CHROM line")
    return parse_program_arguments(p, argv)


def main(argv=None):
    args = get_args(argv)
    with open(args.vcf_list) as f:
        vcf_list = [line.rstrip() for line in f]
    call = dict(master=args.master, sum_quals=args.sum_quals, afreq=args.afreq, safe=args.safe, keep_contigs=args.keep_contigs,
                engine=args.engine, device=args.device)
    return run_program(args, PasteError, lambda out: paste(vcf_list, vcf_out=out, **call))


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

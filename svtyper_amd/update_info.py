"""`python -m svtyper_amd.update_info`: INFO's PE, SR, SU and MSQ of a cohort VCF from the genotyper's per-sample evidence.

    update_info(vcf_in, vcf_out=sys.stdout, engine="host", device=0, file_date=None, keep_contigs=False, block_bytes=None, stats=None)

The step between `svtyper_amd.paste` and `svtyper_amd.classify` in the reference's cohort workflow: scripts/update_info.py (a
positional VCF or stdin; the output is that script's, byte for byte, but for the `##fileDate=` line, which is `file_date`,
YYYYMMDD, default today).  The script is the specification, quirks included: nothing is written before the first body line; the
header is rebuilt from the attributes of its ##INFO, ##ALT and ##FORMAT lines, without SNAME and with MSQ, and everything else is
dropped; every line is written again field by field (POS through int(), QUAL '%0.2f', INFO and FORMAT in the header's order) with
PE the sum of the samples' AP, SR the sum of their AS, SU the sum of both and MSQ the mean SQ of the samples whose GT is neither
"0/0" nor "./." ('%0.2f', or "." where there is none), SQ added in sample order.

Not in the reference: `-o`, `keep_contigs` (the input's ##contig lines stay, directly before the #CHROM line, so that the result
can be sorted by declared rank and written as BCF; as in svtyper_amd.paste), `engine` ("host": the native host twin; "device":
the HIP kernel of svtyper_amd/csrc/svt_vcf_update_info_kernel.h; the same records, byte for byte, and the same text), gzip input
(a path ending in .gz, or whatever begins 1f 8b), BCF input (a path ending in .bcf, or BGZF with the BCF magic: bcf_in.open_text,
decoded by `engine`), and the output options of the other programs (--bgzf / --bcf, --sort, --tabix /
--csi, --deflate, --huffman).

Where the script dies with a traceback, UpdateInfoError names the file, the 1-based line, the sample and the key or token in the
way (`reference`: the script's exception); where it prints a message (a FORMAT key the header does not declare, a line of seven
columns), the CLI prints the same message; both end with status 1, the lines in front of that line written.  Two departures: an SQ
of a positive sample that float() reads as nan or inf raises UpdateInfoError (the script writes MSQ=nan or inf), and so does an AP,
AS or sum beyond int64 (the script goes on with long integers).

The header runs in Python; the body goes through the native library in blocks of at most `block_bytes` of text (None:
cohort.BLOCK_BYTES[engine]): the per-line records from either engine, the output text from one C++ writer.
"""
from __future__ import annotations

import argparse
import sys
import time
from typing import Optional

from . import native_reads as nr
from .cohort import (COLUMNS_MESSAGE, FORMAT_MESSAGE, add_attributes, add_program_arguments, bad_line, begin_body, blocks, bytes_lines,
                     chrom_lines, finish_block, format_table, header_attributes, info_table, open_source, parse_program_arguments,
                     run_options, run_program, run_stats)

MSQ = ["MSQ", "1", "Float", "Mean sample quality of positively genotyped samples"]
# the script's exception and what to say for each way a line can end the run (native_reads.UPDATE_INFO_BAD_*)
_KINDS = {nr.UPDATE_INFO_BAD_COLUMNS: ("IndexError", "fewer than seven columns"),
          nr.UPDATE_INFO_BAD_POS: ("ValueError", "a POS that is no integer: %(text)s"),
          nr.UPDATE_INFO_BAD_QUAL: ("ValueError", "a QUAL that is no number: %(text)s"),
          nr.UPDATE_INFO_BAD_FORMAT: (None, "a FORMAT key the header does not declare: %(text)s"),
          nr.UPDATE_INFO_BAD_KEY: ("KeyError", "%(where)s has no %(text)s"),
          nr.UPDATE_INFO_BAD_NUMBER: ("ValueError", "%(where)s has an AP, AS or SQ that is no number: %(text)s"),
          nr.UPDATE_INFO_BAD_NONFINITE: (None, "%(where)s has an SQ that is not finite: %(text)s"),
          nr.UPDATE_INFO_BAD_OVERFLOW: (None, "%(where)s has a count beyond 64 bits: %(text)s"),
          nr.UPDATE_INFO_BAD_EIGHT: (None, "seven columns where eight are read")}
_VERBATIM = {nr.UPDATE_INFO_BAD_FORMAT: lambda text: FORMAT_MESSAGE % text, nr.UPDATE_INFO_BAD_EIGHT: lambda text: COLUMNS_MESSAGE}


class UpdateInfoError(Exception):
    """the input cannot be rewritten: `file` names it, `line` is the 1-based number of the line in the way, `sample` the sample and
    `token` the key or token, where there is one; `reference`: the exception the script dies of there (None: it goes on, or prints
    `verbatim` and ends with status 1)"""

    def __init__(self, message, file=None, line=None, sample=None, token=None, reference=None, verbatim=None):
        super().__init__(message)
        self.file, self.line, self.sample, self.token, self.reference, self.verbatim = file, line, sample, token, reference, verbatim


_bad = bad_line(UpdateInfoError, _KINDS, _VERBATIM, ("sample", "token"))


def update_info(vcf_in, vcf_out=sys.stdout, engine="host", device=0, file_date=None, keep_contigs=False, block_bytes=None,
                stats: Optional[dict] = None):
    """`vcf_in`: a path (one ending in .gz or beginning with gzip's two bytes is read through gzip) or an open file.  `vcf_out`: any
    text sink the drivers accept; it is not closed.  `stats`, a dict, receives lines, blocks, host_lines (the lines the host's plain
    C++ computed), results (the per-line records of every block, native_reads.UPDATE_INFO_LINE) and, for engine="device", times
    (the sums of vcf_update_info_last_times)."""
    block_bytes = run_options(engine, block_bytes)
    stats = run_stats(stats, lines=0, blocks=0, host_lines=0, results=[], times={})
    name, f, own = open_source(vcf_in, sniff=True, engine=engine, device=device)
    try:
        _run(name, bytes_lines(f), vcf_out, device if engine == "device" else None, file_date or time.strftime("%Y%m%d"), block_bytes, stats,
             keep_contigs)
    finally:
        if own:
            f.close()


def header_tables(header):
    """what the output header is made of, from the input's header lines (one with a single '#' among them): (fileformat, reference,
    the INFO table without SNAME and with MSQ, behind the others unless it is declared, the ALT table, the FORMAT table with the
    script's GT first, the samples)"""
    file_format, reference, _filters, infos, alts, formats = header_attributes([h.rstrip("\n") for h in header if h.startswith("##")], UpdateInfoError)
    add_attributes(infos, MSQ, 4, UpdateInfoError)
    return file_format, reference, [i for i in infos if i[0] != "SNAME"], alts, formats, chrom_lines(header)[-1].rstrip().split("\t")[9:]


def _run(name, lines, vcf_out, device, file_date, block_bytes, stats, keep_contigs):
    body = begin_body(name, lines, vcf_out, file_date, keep_contigs, header_tables, UpdateInfoError)
    if body is None:
        return
    done, first, samples, infos, formats = body                 # done: lines of the file in front of the block
    info_bytes, format_bytes = info_table(infos), format_table(formats)
    for block in blocks(first, lines, block_bytes):
        text = b"".join(block) + (b"" if block[-1].endswith(b"\n") else b"\n")     # (the file's last line: rewritten lines end in a newline)
        finish_block(name, done, block, text, samples, nr.vcf_update_info(text, len(samples), format_bytes, device),
                     lambda kept, results: nr.vcf_update_info_write(kept, len(samples), info_bytes, format_bytes, results),
                     nr.vcf_update_info_last_times if device is not None else None, _bad, vcf_out, stats)
        done += len(block)


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-update-info", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-update-info\ndescription: Update the PE SR fields after SVTyper"))
    p.add_argument(metavar="vcf", dest="vcf_in", nargs="?", type=str, default=None, help="VCF input, gzip where it is (default: stdin)")
    add_program_arguments(p, "where the samples are added up: the native host code or the GPU (same output bytes) [host]")
    return parse_program_arguments(p, argv, "vcf_in")


def main(argv=None):
    args = get_args(argv)
    vcf_in = args.vcf_in if args.vcf_in is not None else sys.stdin.buffer
    return run_program(args, UpdateInfoError, lambda out: update_info(vcf_in, vcf_out=out, engine=args.engine, device=args.device,
                                                                      keep_contigs=args.keep_contigs))


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

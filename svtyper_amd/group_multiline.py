"""`python -m svtyper_amd.group_multiline`: the BND mates of a VCF brought together, in front of `svtyper_amd.paste`.

    group_multiline(vcf_in, vcf_out=sys.stdout, engine="host", device=0, file_date=None, keep_contigs=False, stats=None, hash_bits=64)

The step in front of the paste in the reference's cohort workflow: scripts/vcf_group_multiline.py ("Group multiline variants prior
vcf_paste.py": the paste joins files by line number alone, so a master or sites file has to carry each BND pair as two adjacent
lines).  The output is that script's, byte for byte, but for the `##fileDate=` line, which is `file_date`, YYYYMMDD, default today.
The script is the specification, quirks included: nothing is written before the first body line; the header is rebuilt from the
attributes of its ##INFO, ##ALT and ##FORMAT lines, the script's thirteen genotype FORMAT lines behind the declared ones, and
everything else is dropped; every line is written again field by field (POS through int(), QUAL '%0.2f', INFO and FORMAT in the
header's order).  A line that is no BND is written in place, after END, CIPOS and CIEND were read as integers.  A BND whose MATEID
names a breakend stored earlier is the second of a pair: the stored line is written, then this one with the STORED line's QUAL,
FORMAT and sample columns, both at the place of the second; any other BND is stored under its ID, the last store of an ID
winning, and nothing is written.  Nothing is ever removed, so a third line that names a stored ID writes it again, and a BND
nobody names is dropped silently.

THE WHOLE BODY IS HELD, as the sorted writers hold their output: a pair may span the file, so there are no blocks here.

Not in the reference: `-o`, `keep_contigs` (the input's ##contig lines stay, directly before the #CHROM line), `engine` ("host":
the native host twin; "device": the HIP kernels of svtyper_amd/csrc/svt_vcf_group_kernel.h, a hash join over the IDs of the
whole file; the same records and the same plan, byte for byte, and the same text), gzip and BCF input as in
svtyper_amd.update_info, and the output options of the other programs (--bgzf / --bcf, --sort, --tabix / --csi, --deflate,
--huffman).  `hash_bits` (1..64): the bits of the ID hashes the device sorts by; fewer make IDs collide, for tests.

Where the script dies with a traceback, GroupError names the file, the 1-based line and the key or token in the way (`reference`:
the script's exception); where it prints a message (a FORMAT key the header does not declare, a line of seven columns), the CLI
prints the same message; both end with status 1, the lines in front of that line written.
"""
from __future__ import annotations

import argparse
import sys
import time
from typing import Optional

from . import native_reads as nr
from .cohort import (COLUMNS_MESSAGE, FORMAT_MESSAGE, add_attributes, add_program_arguments, bad_line, begin_body, bytes_lines, chrom_lines,
                     format_table, header_attributes, info_table, open_source, parse_program_arguments, run_options, run_program, run_stats)

# the FORMAT lines the script declares behind the header's own, unless they are declared
FORMATS = [("GQ", "1", "Float", "Genotype quality"),
           ("SQ", "1", "Float", "Phred-scaled probability that this site is variant (non-reference in this sample"),
           ("GL", "G", "Float", "Genotype Likelihood, log10-scaled likelihoods of the data given the called genotype for each possible "
            "genotype generated from the reference and alternate alleles given the sample ploidy"),
           ("DP", "1", "Integer", "Read depth"),
           ("RO", "1", "Integer", "Reference allele observation count, with partial observations recorded fractionally"),
           ("AO", "A", "Integer", "Alternate allele observations, with partial observations recorded fractionally"),
           ("QR", "1", "Integer", "Sum of quality of reference observations"),
           ("QA", "A", "Integer", "Sum of quality of alternate observations"),
           ("RS", "1", "Integer", "Reference allele split-read observation count, with partial observations recorded fractionally"),
           ("AS", "A", "Integer", "Alternate allele split-read observation count, with partial observations recorded fractionally"),
           ("RP", "1", "Integer", "Reference allele paired-end observation count, with partial observations recorded fractionally"),
           ("AP", "A", "Integer", "Alternate allele paired-end observation count, with partial observations recorded fractionally"),
           ("AB", "A", "Float", "Allele balance, fraction of observations from alternate allele, QA/(QR+QA)")]
# the script's exception and what to say for each way a line can end the run (native_reads.GROUP_BAD_*)
_KINDS = {nr.GROUP_BAD_COLUMNS: ("IndexError", "fewer than seven columns"),
          nr.GROUP_BAD_POS: ("ValueError", "a POS that is no integer: %(text)s"),
          nr.GROUP_BAD_QUAL: ("ValueError", "a QUAL that is no number: %(text)s"),
          nr.GROUP_BAD_FORMAT: (None, "a FORMAT key the header does not declare: %(text)s"),
          nr.GROUP_BAD_KEY: ("KeyError", "INFO has no %(text)s"),
          nr.GROUP_BAD_NUMBER: ("ValueError", "END, CIPOS or CIEND holds a token that is no integer: %(text)s"),
          nr.GROUP_BAD_BARE: ("AttributeError", "INFO's %(text)s has no value"),
          nr.GROUP_BAD_ALT: ("IndexError", "a BND pair with an empty ALT"),
          nr.GROUP_BAD_EIGHT: (None, "seven columns where eight are read")}
_VERBATIM = {nr.GROUP_BAD_FORMAT: lambda text: FORMAT_MESSAGE % text, nr.GROUP_BAD_EIGHT: lambda text: COLUMNS_MESSAGE}


class GroupError(Exception):
    """the input cannot be grouped: `file` names it, `line` is the 1-based number of the line in the way (the second line of a pair
    where the pair is), `token` the key or token, where there is one; `reference`: the exception the script dies of there (None:
    it prints `verbatim` and ends with status 1)"""

    def __init__(self, message, file=None, line=None, token=None, reference=None, verbatim=None):
        super().__init__(message)
        self.file, self.line, self.token, self.reference, self.verbatim = file, line, token, reference, verbatim


_bad = bad_line(GroupError, _KINDS, _VERBATIM, ("token",))


def group_multiline(vcf_in, vcf_out=sys.stdout, engine="host", device=0, file_date=None, keep_contigs=False, stats: Optional[dict] = None,
                    hash_bits=64):
    """`vcf_in`: a path (one ending in .gz or beginning with gzip's two bytes is read through gzip, a BCF as its text) or an open
    file.  `vcf_out`: any text sink the drivers accept; it is not closed.  `stats`, a dict, receives lines (read in front of the
    line the script dies on, or all), written (output lines), host_lines (the lines the host's plain C++ decided), host_join
    (the join ran on the host: always for engine="host"), records and plan (native_reads.GROUP_LINE, GROUP_OUT) and, for
    engine="device", times (vcf_group_last_times)."""
    run_options(engine)
    stats = run_stats(stats, lines=0, written=0, host_lines=0, host_join=False, records=None, plan=None, times={})
    name, f, own = open_source(vcf_in, sniff=True, engine=engine, device=device)
    try:
        _run(name, bytes_lines(f), vcf_out, device if engine == "device" else None, file_date or time.strftime("%Y%m%d"), stats, keep_contigs,
             hash_bits)
    finally:
        if own:
            f.close()


def header_tables(header):
    """what the output header is made of, from the input's header lines: (fileformat, reference, the INFO table, the ALT table, the
    FORMAT table with the script's GT first and its thirteen genotype fields behind the declared ones, the samples)"""
    file_format, reference, _filters, infos, alts, formats = header_attributes([h.rstrip("\n") for h in header if h.startswith("##")], GroupError)
    for row in FORMATS:
        add_attributes(formats, row, 4, GroupError)
    return file_format, reference, infos, alts, formats, chrom_lines(header)[-1].rstrip().split("\t")[9:]


def _run(name, lines, vcf_out, device, file_date, stats, keep_contigs, hash_bits):
    begun = begin_body(name, lines, vcf_out, file_date, keep_contigs, header_tables, GroupError)
    if begun is None:
        return
    done, first, samples, infos, formats = begun
    info_bytes, format_bytes = info_table(infos), format_table(formats)
    body = [first] + list(lines)                    # the whole body: a pair may span it
    text = b"".join(body) + (b"" if body[-1].endswith(b"\n") else b"\n")
    records, plan, report = nr.vcf_group(text, len(samples), format_bytes, device, hash_bits)
    out, _out_off, written = nr.vcf_group_write(text, len(samples), info_bytes, format_bytes, records, plan)
    vcf_out.write(out.decode("utf-8", "surrogateescape"))
    stats.update(lines=report["bad_line"] - 1 if report["bad_line"] else len(records), written=len(plan), host_lines=report["host_lines"],
                 host_join=bool(report["host_join"]), records=records, plan=plan)
    if device is not None:
        stats["times"] = nr.vcf_group_last_times()
    if written["bad_line"]:                         # (a plan that is not the text's: neither engine makes one)
        raise GroupError("%s: entry %d of the plan cannot be written" % (name, written["bad_line"]), name)
    if report["bad_line"]:
        raise _bad(name, done + report["bad_line"], report["bad_kind"], report["bad_text"])


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-group-multiline", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-group-multiline\ndescription: Group multiline variants prior vcf_paste.py"))
    p.add_argument(metavar="vcf", dest="vcf_in", nargs="?", type=str, default=None, help="VCF input, gzip where it is (default: stdin)")
    add_program_arguments(p, "where the mates are joined: the native host code or the GPU (same output bytes) [host]")
    return parse_program_arguments(p, argv, "vcf_in")


def main(argv=None):
    args = get_args(argv)
    vcf_in = args.vcf_in if args.vcf_in is not None else sys.stdin.buffer
    return run_program(args, GroupError, lambda out: group_multiline(vcf_in, vcf_out=out, engine=args.engine, device=args.device,
                                                                     keep_contigs=args.keep_contigs))


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

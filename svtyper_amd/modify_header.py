"""`python -m svtyper_amd.modify_header`: add an INFO, FORMAT or FILTER line to a VCF's header, or only normalise the header.

    modify_header(vcf_in, vcf_out=sys.stdout.buffer, vcf_id=None, category=None, type=None, number=None, description=None,
                  file_date=None, keep_contigs=False)

The reference's scripts/vcf_modify_header.py (-i ID -c INFO|FORMAT|FILTER -t TYPE -n NUMBER -d DESCRIPTION [vcf]); the output is
that script's, byte for byte, but for the `##fileDate=` line, which is `file_date`, YYYYMMDD, default today.  The script is the
specification: nothing is written for a file without a body line; the header is rebuilt as the other cohort programs rebuild it
(fileformat, fileDate, reference, then the FILTER, INFO, ALT and FORMAT lines from their attributes, the script's GT first;
everything else is dropped, and the #CHROM line loses FORMAT where there are no samples), here WITH the ##FILTER lines, whose
attributes the script cuts two characters in front of the line's end.  `-c INFO` removes an INFO of that ID and appends the new
one; `-c FORMAT` and `-c FILTER` add theirs only if the ID is not declared; any other category, or none, leaves the tables alone.
An option that is not given reads "None", as str() of the script's default does.  The body is copied verbatim, in binary: it is
not parsed, which is why the output options of the other programs are not offered.

Not in the reference: `-o`, `keep_contigs` (the input's ##contig lines stay, directly before the #CHROM line) and gzip or BCF
input (cohort.open_source).  Pure Python: there is no native code and no GPU here.
"""
from __future__ import annotations

import argparse
import sys
import time

from .cohort import (_unquoted, add_attributes, bytes_lines, chrom_lines, declared_lines, header_attributes, header_text, open_source,
                     read_header)


class ModifyHeaderError(Exception):
    """the header cannot be rebuilt: `reference` is the exception the script dies of (None: a header line it cannot read)"""

    def __init__(self, message, reference=None):
        super().__init__(message)
        self.reference = reference


def modified_tables(header, vcf_id=None, category=None, type=None, number=None, description=None):
    """(fileformat, reference, the FILTER, INFO, ALT and FORMAT tables with the change made, the samples) of the input's header lines"""
    file_format, reference, filters, infos, alts, formats = header_attributes([h.rstrip("\n") for h in header if h.startswith("##")], ModifyHeaderError)
    vcf_id, type, number, description = (str(v) for v in (vcf_id, type, number, description))
    if category == "INFO":
        for row in infos:
            if row[0] == vcf_id:
                infos.remove(row)
                break
        add_attributes(infos, (vcf_id, number, type, description), 4, ModifyHeaderError)
    elif category == "FORMAT":
        add_attributes(formats, (vcf_id, number, type, description), 4, ModifyHeaderError)
    elif category == "FILTER":
        add_attributes(filters, (vcf_id, description), 2, ModifyHeaderError)
    return file_format, reference, filters, infos, alts, formats, chrom_lines(header)[-1].rstrip().split("\t")[9:]


def modify_header(vcf_in, vcf_out=None, vcf_id=None, category=None, type=None, number=None, description=None, file_date=None, keep_contigs=False):
    """`vcf_in`: a path or an open file, as the other cohort programs take it.  `vcf_out`: a BINARY sink (default: stdout's); it is
    not closed."""
    if vcf_out is None:
        vcf_out = sys.stdout.buffer
    name, f, own = open_source(vcf_in, sniff=True)
    try:
        lines = bytes_lines(f)
        header, first = read_header(lines)
        if first is None:                           # (the header is written when the first body line is met)
            return
        if not chrom_lines(header):                 # (the script's sample list is never bound)
            raise ModifyHeaderError("%s, line %d: a body line and no #CHROM line in front of it" % (name, len(header) + 1), "UnboundLocalError")
        file_format, reference, filters, infos, alts, formats, samples = modified_tables(header, vcf_id, category, type, number, description)
        declared = ['##FILTER=<ID=%s,Description="%s">' % (i, _unquoted(d)) for i, d in filters] + declared_lines(infos, alts, formats)
        text = header_text(file_format, file_date or time.strftime("%Y%m%d"), reference, declared, header, samples, keep_contigs, with_format=bool(samples))
        vcf_out.write(text.encode("utf-8", "surrogateescape"))
        vcf_out.write(first)
        for line in lines:
            vcf_out.write(line)
    finally:
        if own:
            f.close()


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-modify-header", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-modify-header\ndescription: Add or modify a VCF header line"))
    p.add_argument("-i", "--id", dest="vcf_id", metavar="STR", type=str, required=False, help="field id")
    p.add_argument("-c", "--category", dest="category", metavar="STR", type=str, help="INFO, FORMAT, FILTER")
    p.add_argument("-t", "--type", dest="type", metavar="STR", type=str, required=False, help="Number, String, Float, Integer")
    p.add_argument("-n", "--number", dest="number", metavar="STR", type=str, required=False, help="integer, A, R, G, or .")
    p.add_argument("-d", "--description", dest="description", metavar="STR", type=str, required=False, help="description")
    p.add_argument(metavar="vcf", dest="vcf_in", nargs="?", type=str, default=None, help="VCF input, gzip where it is (default: stdin)")
    p.add_argument("--keep-contigs", dest="keep_contigs", action="store_true",
                   help="keep the input's ##contig lines, directly before the #CHROM line")
    p.add_argument("-o", "--output_vcf", metavar="FILE", type=argparse.FileType("wb"), default=None, help="output VCF to write (default: stdout)")
    args = p.parse_args(argv)
    if args.vcf_in is None and sys.stdin.isatty():
        p.print_help()
        sys.exit(1)
    return args


def main(argv=None):
    args = get_args(argv)
    out = args.output_vcf if args.output_vcf is not None else sys.stdout.buffer
    try:
        modify_header(args.vcf_in if args.vcf_in is not None else sys.stdin.buffer, out, args.vcf_id, args.category, args.type, args.number,
                      args.description, keep_contigs=args.keep_contigs)
        out.flush()
    except ModifyHeaderError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    return 0


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

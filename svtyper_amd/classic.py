"""`svtyper` (multi-sample) driver with the reference's call surface.

    sv_genotype(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp,
                lib_info_path, debug, alignment_outpath, ref_fasta, sum_quals, max_reads, max_ci_dist)

Same arguments, defaults and output bytes as svtyper/classic.py:107-533, but the per-sample
likelihood block (classic.py:286-513) does not run here: evidence is packed on the host and
genotyped in device batches (pipeline.py).  The run itself is driver.Driver, shared with `svtyper-sso`; `Classic` below holds
what this program does its own way.  `engine` is an extra, keyword-only seam; it
defaults to the HIP library and there is no CPU implementation in this package.
"""
from __future__ import annotations

import argparse
import functools
import json
import logging
import os
import sys
from itertools import chain

from . import __version__, sharded
from . import evidence as ev
from .bam import check_deflate, check_huffman
from .bulk_vcf import QUAL_CLASSIC
from .driver import Driver, parse_arguments, run_cli, run_main
from .library import Sample, write_sample_json
from .native_reads import COUNT_CLASSIC
from .pipeline import SampleColumnWriter, add_read_to, fetch_window, text_blocks
from .results import results_to_dicts
from .vcf import Variant

CHUNK_UNITS = 50_000    # (breakpoint, sample) units per device batch: small enough to overlap chunks (ChunkPipeline)


def gather_all_reads(sample: Sample, bp: dict, max_reads):
    """Fragments of both breakends, or ({}, True) when a side has more than max_reads reads
    (classic.py:54-100: the counter runs over every fetched record of that side)."""
    fragments = {}
    for side in ("A", "B"):
        chrom, lo, hi = fetch_window(sample, bp[side]["chrom"], bp[side]["pos"], bp[side]["ci"], as_int=False)
        for i, read in enumerate(sample.bam.fetch(chrom, lo, hi)):
            if read.is_unmapped or read.is_duplicate:
                continue
            lib = sample.get_lib(read.get_tag("RG"))
            if lib.name not in sample.active_libs:
                continue
            if max_reads is not None and i > max_reads:
                return {}, True
            add_read_to(fragments, read, lib)
    return fragments, False


_FORMAT_KEYS = ("GL", "DP", "RO", "AO", "QR", "QA", "RS", "AS", "ASC", "RP", "AP", "AB", "GQ", "SQ", "GT")


def apply_result(var: Variant, sample_name: str, gt: int, res: dict) -> None:
    """Result of one unit -> FORMAT fields and QUAL of one sample (classic.py:454-513)."""
    g = var.genotype(sample_name)
    if gt == ev.GT_SKIPPED:                       # classic.py:282-284
        g.set_format("GT", "./.")
        return
    f = res["formats"]
    if gt == ev.GT_BLANK:                         # classic.py:496-513 (QUAL is reset, not kept)
        var.qual = 0
    g.set_formats([(key, f[key]) for key in _FORMAT_KEYS])
    if gt >= 0:
        var.qual += res["qual"]                   # classic.py:485


class Classic(Driver):
    """What `svtyper` does its own way (driver.Driver is the run it shares with `svtyper-sso`)."""
    count_mode = COUNT_CLASSIC          # classic.py:54-100: the max_reads counter runs over every fetched record of a side
    site_quals = True                   # classic.py:216-217,485,498: QUAL is one number over a site's samples, so the pass is given
    qual_mode = QUAL_CLASSIC            # the incoming QUAL of every site, and the bulk route writes QUAL by the same rule
    skip_hash_lines = False             # classic.py:191-199: behind the header every line is a variant line
    bulk_under_debug = False            # classic.py:410-419 prints per (site, sample); the bulk route has no such print

    def alignment_paths(self):
        """classic.py:122-132: a comma list; a name that is no *.bam / *.cram ends the program with status 1"""
        for path in self.bam_string.split(","):
            if not (path.endswith(".bam") or path.endswith(".cram")):
                sys.stderr.write("Error: %s is not a valid alignment file (*.bam or *.cram)\n" % path)
                sys.exit(1)
            yield path

    def read_library_file(self):
        """classic.py:136-140"""
        if self.lib_info_path is not None and os.path.isfile(self.lib_info_path):
            with open(self.lib_info_path) as f:
                return json.load(f)

    def write_library_file(self):
        """classic.py:168-174"""
        if self.lib_info_path is not None and not os.path.isfile(self.lib_info_path):
            logging.info("Writing library metrics to %s..." % self.lib_info_path)
            write_sample_json(self.samples, open(self.lib_info_path, "w"))

    def open_vcf(self, bulk):
        """classic.py:191-210: every '#' line in front of the body is header, and the first variant line ends it -- an
        input without one gets no header.  Samples the VCF does not name are added behind the ones it does; with other
        samples' columns in the VCF every line keeps its Genotype objects, so the whole body goes per line."""
        vcf, vcf_in = self.vcf, self.vcf_in
        header_lines, first = [], None
        for line in vcf_in:
            if line[0] != "#":
                first = line
                break
            header_lines.append(line)
        if first is None:
            return None, None
        vcf.add_header(header_lines)
        vcf.add_custom_svtyper_headers()
        for sample in self.samples:
            if sample.name not in vcf.sample_list:
                vcf.add_sample(sample.name)
        self.vcf_out.write(vcf.get_header() + "\n")
        self.fast = SampleColumnWriter(vcf, [s.name for s in self.samples], skipped_as_dots=True)    # classic.py:282-284
        if bulk and self.fast.enabled and hasattr(vcf_in, "readline"):
            return None, text_blocks(first, vcf_in, len(self.samples))      # blocks read from the stream as they are needed
        return chain((first,), vcf_in), None

    def warn(self, text):
        """classic.py:223,229"""
        sys.stderr.write(text)

    def gather(self, sample, bp, max_reads):
        return gather_all_reads(sample, bp, max_reads)

    def render_actions(self, results, actions):
        """the output text of every action, one string each (the lines of a variant, of a BND pair, of a line passed through)"""
        fast, samples, debug = self.fast, self.samples, self.debug
        n_samp = len(samples)
        gts = results.gt.tolist()
        site_qual = None if results.site_qual is None else results.site_qual.tolist()
        columns = sqs = dicts = None
        for action in actions:
            if action[0] == "raw":
                yield action[1].get_var_string() + "\n"
                continue
            _, var, var2, first_unit = action
            unit_gts = gts[first_unit:first_unit + n_samp]
            if (not debug and fast.eligible(var)
                    and any(g != ev.GT_SKIPPED for g in unit_gts)):
                # bulk path: the sample columns of the whole chunk were formatted in one native call
                if columns is None:
                    columns = fast.columns(results)
                    sqs = results.sq.tolist()
                if site_qual is not None:
                    var.qual = site_qual[first_unit // n_samp]
                else:
                    for k, g in enumerate(unit_gts):           # classic.py:485,498
                        if g >= 0:
                            var.qual += sqs[first_unit + k]
                        elif g == ev.GT_BLANK:
                            var.qual = 0
                cols = columns[first_unit:first_unit + n_samp]
                text = var.get_var_string_with(fast.format_string, cols) + "\n"
                if var2 is not None:               # BND: second mate carries the same QUAL and genotypes
                    var2.qual = var.qual
                    text += var2.get_var_string_with(fast.format_string, cols) + "\n"
                yield text
                continue
            if dicts is None:
                dicts = results_to_dicts(results)
            for k, sample in enumerate(samples):
                if debug:
                    _debug_print(results.rec[first_unit + k])
                apply_result(var, sample.name, gts[first_unit + k], dicts[first_unit + k])
            if site_qual is not None:      # the same running sum, over the refined SQ (hip.site_qual_host)
                var.qual = site_qual[first_unit // n_samp]
            text = var.get_var_string() + "\n"
            if var2 is not None:                   # BND: second mate carries the same genotypes
                var.share_genotypes_with(var2)
                text += var2.get_var_string() + "\n"
            yield text

    def finish(self, unpaired):
        """classic.py:530-533"""
        if unpaired:
            logging.warning("Unpaired breakends found in file. These will not be present in output.")
        self.vcf_in.close()
        self.vcf_out.close()


def sv_genotype(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp, lib_info_path,
                debug, alignment_outpath, ref_fasta, sum_quals, max_reads, max_ci_dist, *, engine=None, geometry="host",
                reader=None, stats=None, inflate="host", library_scan="host", verify="off", deflate="zlib", huffman="fixed",
                alignment_sort=False, alignment_index=None, alignment_out=None, cram_codec=None):
    """`alignment_outpath` (-w): the reads that entered the tallies go to a BAM, tagged XV:A:R / XV:A:A as the reference tags them
    (driver.tag_and_write; the tags that depend on p_concordant come from the device, svt_batch_verdicts).  Legal with
    reader="python" (what reader=None then means) or reader="device" (the reads are cut and tagged on the GPU: the evidence dump of
    svt_bam_evidence_device_dump; the default engine, or one with supports_dump) and geometry="host"; ValueError otherwise, and for
    an engine without supports_verdicts.  `deflate`: who compresses that BAM's members -- "zlib", or the library's own compressor on
    the "host" or on the "device" (bam.BgzfWriter; the same inflated bytes and member boundaries); ValueError for anything else.  `huffman`: "fixed", or "dynamic" for
    dynamic-Huffman blocks from that compressor (ValueError with deflate="zlib").  `alignment_sort` (--sort-alignment): that BAM in
    stable coordinate order, its header saying SO:coordinate; `alignment_index="bai"` (--bai): its index beside it, at
    alignment_outpath + ".bai"; `alignment_index="csi"` (--alignment-csi): a CSI index instead, at alignment_outpath + ".csi", which
    also holds records beyond 2^29 (bam.AlignmentFile's sort= / index= / csi=: both hold every record until the end; BamOrderError for records
    that cannot be sorted or indexed).  `cram_codec` ("host" | "device"; None = "host"): with a *.cram among the alignment files, who
    decodes its rANS blocks (cram.py; pipeline.check_cram has the usage errors of a CRAM input).  ValueError for either without `alignment_outpath`.  `alignment_out`: a writer that takes the
    dump's records instead of a file opened at `alignment_outpath` (write / write_raw / close, e.g. bam.RecordSink: what
    sharded.sv_genotype_sharded gives every rank); the checks above apply as they do to a path."""
    check_huffman(huffman, check_deflate(deflate))
    run = Classic(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp, lib_info_path, debug, ref_fasta,
                  sum_quals, max_reads, max_ci_dist)
    run.alignment_outpath = alignment_outpath
    run.deflate = deflate
    run.huffman = huffman
    run.alignment_sort = bool(alignment_sort)
    run.alignment_index = alignment_index
    run.alignment_out = alignment_out
    run.cram_codec = cram_codec
    return run.run(CHUNK_UNITS, engine=engine, geometry=geometry, reader=reader, stats=stats, inflate=inflate,
                   library_scan=library_scan, verify=verify)


def _debug_print(rec):
    t = dict(zip(ev.TALLY_NAMES, (float(x) for x in rec["tallies"])))
    print("--------------------------")
    for key in ("ref_span", "alt_span", "ref_seq", "alt_seq", "alt_clip"):
        print("%s: %s" % (key, t[key]))
    if int(rec["gt"]) not in (ev.GT_BLANK, ev.GT_SKIPPED):
        print([float(x) for x in rec["gl"]])


# ------------------------------------------------------------------------------------------ CLI
def get_args():
    p = argparse.ArgumentParser(formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper (MI355X-native likelihood path)\nversion: %s\n"
        "description: Compute genotype of structural variants based on breakpoint depth" % __version__))

    def own(p):
        p.add_argument("-w", "--write_alignment", metavar="FILE", dest="alignment_outpath", type=str, default=None,
                       help="write relevant reads to BAM file")
        p.add_argument("--verbose", action="store_true", default=False, help="Report status updates")
        # the `-w` BAM in coordinate order / with its .bai beside it (README; bam.AlignmentFile: sort=, index="bai").  Not listed by
        # --help, like --sort and --tabix: the help text is pinned byte for byte.
        p.add_argument("--sort-alignment", dest="alignment_sort", action="store_true", help=argparse.SUPPRESS)
        p.add_argument("--bai", dest="alignment_bai", action="store_true", help=argparse.SUPPRESS)
        p.add_argument("--alignment-csi", dest="alignment_csi", action="store_true", help=argparse.SUPPRESS)
        # under torch.distributed.run: the ranks' dumps gathered onto rank 0, which writes the one `-w` BAM (sharded.sv_genotype_sharded)
        p.add_argument("--gather-alignment", dest="alignment_gather", action="store_true", help=argparse.SUPPRESS)
    args = parse_arguments(p, "BAM or CRAM file(s), comma-separated if genotyping multiple samples", None, own)
    if (args.alignment_sort or args.alignment_bai) and args.alignment_outpath is None:
        p.error("--sort-alignment and --bai need -w/--write_alignment")
    if args.alignment_csi and args.alignment_outpath is None:
        p.error("--alignment-csi needs -w/--write_alignment")
    if args.alignment_csi and args.alignment_bai:
        p.error("--alignment-csi and --bai name two formats for one index: give one of them")
    if args.alignment_gather and args.alignment_outpath is None:
        p.error("--gather-alignment needs -w/--write_alignment")
    if args.alignment_gather and sharded.job() is None:
        p.error("--gather-alignment is for a run of several ranks under torch.distributed.run: one process writes its dump itself")
    return args


def main():
    args = get_args()
    if args.alignment_outpath is not None:
        if sharded.job() is not None and not args.alignment_gather:
            raise ValueError(sharded.WRITE_ALIGNMENT_SHARDED)
        if args.reader is None:
            args.reader = "python"      # the reader that keeps the reads it tallied (sv_genotype: reader=None with -w)
    logging.basicConfig(format="%(message)s", level=logging.INFO if args.verbose else logging.WARNING)
    call = (args.bam, args.input_vcf, args.output_vcf, args.min_aligned, args.split_weight, args.disc_weight,
            args.num_samp, args.lib_info_path, args.debug, args.alignment_outpath, args.ref_fasta,
            args.sum_quals, args.max_reads, args.max_ci_dist)
    own = dict(deflate=args.deflate, huffman=args.huffman)      # (of this program alone: the `-w` BAM)
    order = dict(alignment_sort=args.alignment_sort, alignment_index="csi" if args.alignment_csi else "bai" if args.alignment_bai else None)
    return run_main(functools.partial(sv_genotype, **own, **order), functools.partial(sharded.sv_genotype_sharded, **own, **order, alignment_gather=args.alignment_gather), call, args)


def cli():
    run_cli(main)


if __name__ == "__main__":
    cli()

"""`svtyper-sso` (single sample) driver with the reference's call surface.

    sso_genotype(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp,
                 lib_info_path, debug, ref_fasta, sum_quals, max_reads, max_ci_dist, cores, batch_size)

Same arguments, defaults and output bytes as svtyper/singlesample.py:764-814.  The reference's
`--cores N` fans batches of breakpoints out to a multiprocessing.Pool (singlesample.py:710-762);
here every breakpoint of a chunk goes to the GPU in one batch instead, so `cores` only selects the
reference's two-pass bookkeeping and `batch_size` is accepted for compatibility.  The kernel runs
with the singlesample floating-point association (SVT_FLAG_SSO_ASSOCIATION).  The run itself is driver.Driver,
shared with `svtyper`; `Sso` below holds what this program does its own way.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

from . import __version__, sharded
from . import evidence as ev
from .bulk_vcf import QUAL_SSO
from .driver import Driver, parse_arguments, run_cli, run_main
from .library import Sample, write_sample_json
from .native_reads import COUNT_SSO
from .pipeline import SampleColumnWriter, add_read_to, block_chars, fetch_window
from .results import results_to_dicts
from .vcf import Variant

CHUNK_UNITS = 50_000    # (breakpoint, sample) units per device batch: small enough to overlap chunks (ChunkPipeline)
_ASSIGN_ORDER = ("GT", "GQ", "SQ", "GL", "DP", "AO", "RO", "AS", "ASC", "RS", "AP", "RP", "QR", "QA", "AB")


def logit(msg):
    import datetime
    import time
    ts = time.strftime("[ %Y-%m-%d %T ]", datetime.datetime.now().timetuple())
    print("%s %s" % (ts, msg), file=sys.stderr)
    sys.stderr.flush()


def gather_reads(sample: Sample, bp: dict, max_reads):
    """Fragments of both breakends, or ({}, True) when either region holds more than max_reads
    countable reads (singlesample.py:158-205: bam.count() of both regions first, then fetch)."""
    regions = [fetch_window(sample, bp[s]["chrom"], bp[s]["pos"], bp[s]["ci"], as_int=True) for s in ("A", "B")]
    if max_reads is not None:
        counts = [sample.bam.count(c, lo, hi, read_callback="all") for c, lo, hi in regions]
        if counts[0] > max_reads or counts[1] > max_reads:
            logit("SKIPPING -- Variant '%s' has a region with too many reads (> %s)" % (bp["id"], max_reads))
            return {}, True
    fragments = {}
    for chrom, lo, hi in regions:
        for read in sample.bam.fetch(chrom, lo, hi):
            if read.is_unmapped or read.is_duplicate:
                continue
            lib = sample.rg_to_lib[read.get_tag("RG")]
            if lib.name not in sample.active_libs:
                continue
            add_read_to(fragments, read, lib)
    return fragments, False


# ------------------------------------------------------------------------------------------
# the reference's inner operator seams, by name: same arguments, same dict shapes,
# the arithmetic on the MI355X through the C ABI (no CPU implementation lives here)
# ------------------------------------------------------------------------------------------
SPLIT_SLOP = 3   # singlesample.py:792 / classic.py:184
_TALLY_KEYS = ("ref_seq", "alt_seq", "alt_clip", "ref_span", "alt_span")   # SVT_TAL_* order


def blank_genotype_result():
    """svtyper/singlesample.py:207-227"""
    from .results import blank_result
    return blank_result()


def _library_table(lib):
    if hasattr(lib, "table"):
        return lib.table()
    return ev.LibraryTable.from_counter(dict(lib.hist), float(lib.mean), float(lib.sd), getattr(lib, "name", "lib"))


def tally_variant_read_fragments(split_slop, min_aligned, breakpoint, sam_fragments, debug, *, device=0):
    """svtyper/singlesample.py:355-404: the five evidence tallies of one breakpoint over its read-fragments
    (sorted by query name, fragment-local split-read sums, zeroing rules applied) as the reference's `counts`
    dict.  The fragments' yes/no geometry is asked here (packer.py), every weight, the insert-size test, the
    sums and the zeroing rules are evaluated by the streaming kernel (svt_genotype, SVT_FLAG_SSO_ASSOCIATION)."""
    from . import hip
    from .packer import BatchBuilder, pack_fragments, unit_header
    libs, lib_index = [], {}
    for name in sorted(sam_fragments.keys()):
        lib = sam_fragments[name].lib
        if id(lib) not in lib_index:
            lib_index[id(lib)] = len(libs)
            libs.append(_library_table(lib))
    if not libs:     # no fragments: the reference's loop body never runs and the initial integer zeros come back
        counts = {k: 0 for k in _TALLY_KEYS}
    else:
        builder = BatchBuilder(libs, 1.0, 1.0)
        builder.add(unit_header(breakpoint), pack_fragments(sam_fragments, breakpoint, lib_index, min_aligned, split_slop))
        res = hip.genotype_batch(builder.build(), device=device, flags=ev.FLAG_SSO_ASSOCIATION)
        counts = {k: float(res.tallies[0, i]) for i, k in enumerate(_TALLY_KEYS)}
    if debug:
        items = ("ref_span", "alt_span", "ref_seq", "alt_seq", "alt_clip")
        logit("{} -- read fragment tally counts:\n{}".format(
            breakpoint["id"], "\n".join("{}: {}".format(i, counts[i]) for i in items)))
    return counts


def bayesian_genotype(breakpoint, counts, split_weight, disc_weight, debug, *, device=0):
    """svtyper/singlesample.py:406-473: `counts` (as tally_variant_read_fragments returned them) -> the
    reference's result dict {'qual', 'formats': {GT, GQ, SQ, GL, DP, AO, RO, AS, ASC, RS, AP, RP, QR, QA, AB}}.
    QR/QA, bayes_gt, the GT/GQ decision and the counts come from svt_genotype_counts (device); SQ is then taken
    from the bit-exact GL with the host libm, as the reference does (svt_results_host_sq)."""
    from . import hip
    from .results import result_from_record
    res = hip.host_sq(hip.genotype_counts([[counts[k] for k in _TALLY_KEYS]], [breakpoint["svtype"] == "DUP"],
                                          split_weight, disc_weight, device))
    if debug:
        logit("{} -- log probabilities (homref, het, homalt) : {}".format(breakpoint["id"], [float(x) for x in res.gl[0]]))
    return result_from_record(res.rec[0])


def assign_genotype(variant: Variant, sample_name: str, res: dict) -> None:
    """singlesample.py:544-575: every FORMAT field is always written; QUAL accumulates."""
    variant.qual += res["qual"]
    f = res["formats"]
    variant.genotype(sample_name).set_formats([(key, f[key]) for key in _ASSIGN_ORDER])


class Sso(Driver):
    """What `svtyper-sso` does its own way (driver.Driver is the run it shares with `svtyper`)."""
    flags = ev.FLAG_SSO_ASSOCIATION     # singlesample.py:246-353: fragment-local split-read sums (and QUAL is the one sample's SQ)
    count_mode = COUNT_SSO              # singlesample.py:158-185: bam.count() of both regions before any fetch
    qual_mode = QUAL_SSO                # singlesample.py:544-546
    skip_hash_lines = True              # singlesample.py's vcf_variants(): every line that does not start with '#'
    # (debug: singlesample.py:401-402,427-428 log inside the two seams below, nothing in the driver -- the bulk route stays)

    def __init__(self, *reference_args, cores):
        super().__init__(*reference_args, n_threads=cores or 0)     # (--cores = the C++ reader's thread count)
        self.cores = cores

    def alignment_paths(self):
        """singlesample.py:49-51,783-784: one absolute path; the message of a bad one is the exit status"""
        path = os.path.abspath(self.bam_string)
        if not (path.endswith(".bam") or path.endswith(".cram")):
            sys.exit("Error: %s is not a valid alignment file (*.bam or *.cram)\n" % path)
        yield path

    def read_library_file(self):
        """singlesample.py:71-76"""
        if self.lib_info_path is not None and os.path.exists(self.lib_info_path):
            logit("Reading library metrics from %s..." % self.lib_info_path)
            with open(self.lib_info_path) as f:
                return json.load(f)

    def write_library_file(self):
        """singlesample.py:86-93"""
        if self.lib_info_path is not None and not os.path.exists(self.lib_info_path):
            logit("Writing library metrics to %s..." % self.lib_info_path)
            write_sample_json(self.samples, open(self.lib_info_path, "w"))

    def open_vcf(self, bulk):
        """singlesample.py:112-125,580: only the '##' lines are parsed, so sample columns of the input are not carried over
        and the BAM's sample becomes the only column; the header is always written.  The input is read whole (the reference
        reads its file three times): as lines, or for the bulk route as one text that is cut into blocks behind the '##' lines."""
        vcf, vcf_in, sample = self.vcf, self.vcf_in, self.samples[0]
        lines = None if bulk else vcf_in.readlines()
        text = vcf_in.read() if bulk else "".join(lines)
        header, input_samples, body_at = [], [], 0
        while text.startswith("##", body_at):
            nl = text.find("\n", body_at)
            end = len(text) if nl < 0 else nl + 1
            header.append(text[body_at:end])
            body_at = end
        at = 0 if text.startswith("#CHROM") else text.find("\n#CHROM") + 1
        if at > 0 or text.startswith("#CHROM"):
            nl = text.find("\n", at)
            input_samples = text[at:len(text) if nl < 0 else nl].rstrip().split("\t")[9:]
        vcf.filename = getattr(vcf_in, "name", "<stdin>")
        vcf.add_header(header)
        vcf.add_custom_svtyper_headers()
        if sample.name not in input_samples:
            logit("Note: Did not find sample name : '%s' in input vcf: '%s' -- adding" % (sample.name, vcf.filename))
        vcf.add_sample(sample.name)
        vcf.write_header(self.vcf_out)
        logit("Genotyping Input VCF (%s Mode)" % ("Serial" if self.cores is None else "Parallel"))     # singlesample.py:804-809
        self.fast = SampleColumnWriter(vcf, [sample.name], skipped_as_dots=False)
        if not bulk:
            return lines, None

        def blocks():
            nl = text.find("\n", body_at)
            chars = block_chars((nl if nl >= 0 else len(text)) - body_at)
            at = body_at
            while at < len(text):
                cut = text.find("\n", at + chars)
                end = len(text) if cut < 0 else cut + 1
                yield text[at:end]
                at = end
        return None, blocks()

    warn = staticmethod(logit)              # singlesample.py:595-609
    gather = staticmethod(gather_reads)     # singlesample.py:158-205

    def render_actions(self, results, actions):
        """the output text of every action, one string each"""
        fast, sample = self.fast, self.samples[0]
        columns = gts = sqs = dicts = None
        for action in actions:
            if action[0] == "raw":
                yield action[1].get_var_string() + "\n"
                continue
            _, variant, variant2, unit = action
            if fast.eligible(variant):
                # bulk path: the sample column of every unit of the chunk was formatted in one native call
                if columns is None:
                    columns, gts, sqs = fast.columns(results), results.gt.tolist(), results.sq.tolist()
                if gts[unit] >= 0:
                    variant.qual += sqs[unit]          # singlesample.py:544-546
                cols = columns[unit:unit + 1]
                out = variant.get_var_string_with(fast.format_string, cols) + "\n"
                if variant2 is not None:
                    variant2.qual = variant.qual
                    out += variant2.get_var_string_with(fast.format_string, cols) + "\n"
                yield out
                continue
            if dicts is None:
                dicts = results_to_dicts(results)   # blank for "no evidence" and "too many reads" alike
            assign_genotype(variant, sample.name, dicts[unit])
            out = variant.get_var_string() + "\n"
            if variant2 is not None:
                variant.share_genotypes_with(variant2)
                out += variant2.get_var_string() + "\n"
            yield out

    def finish(self, unpaired):
        """singlesample.py:814 (first BND mates without a partner are dropped without a word)"""
        self.samples[0].close()


def sso_genotype(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp, lib_info_path,
                 debug, ref_fasta, sum_quals, max_reads, max_ci_dist, cores, batch_size, *, engine=None, geometry="host",
                 reader=None, stats=None, inflate="host", library_scan="host", verify="off", cram_codec=None):
    """`cram_codec` ("host" | "device"; None = "host"): with a *.cram input, who decodes its rANS blocks (cram.py; pipeline.check_cram has
    the usage errors of a CRAM input)."""
    if vcf_in is None:      # singlesample.py:780-781: in front of everything else, the alignment file included
        return
    run = Sso(bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp, lib_info_path, debug, ref_fasta,
              sum_quals, max_reads, max_ci_dist, cores=cores)
    run.cram_codec = cram_codec
    return run.run(CHUNK_UNITS, engine=engine, geometry=geometry, reader=reader, stats=stats, inflate=inflate,
                   library_scan=library_scan, verify=verify)


# ------------------------------------------------------------------------------------------ CLI
def get_args():
    p = argparse.ArgumentParser(formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-sso (MI355X-native likelihood path)\nversion: %s\n"
        "description: Compute genotype of structural variants based on breakpoint depth on a SINGLE sample"
        % __version__))

    def own(p):
        p.add_argument("--cores", type=int, metavar="INT", default=None,
                       help="accepted for compatibility: breakpoints are batched onto the GPU instead of a worker pool")
        p.add_argument("--batch_size", type=int, metavar="INT", default=1000,
                       help="accepted for compatibility with the reference's worker batches")
    return parse_arguments(p, "BAM or CRAM file", 1000, own)


def main():
    args = get_args()
    call = (args.bam, args.input_vcf, args.output_vcf, args.min_aligned, args.split_weight, args.disc_weight,
            args.num_samp, args.lib_info_path, args.debug, args.ref_fasta, args.sum_quals, args.max_reads,
            args.max_ci_dist, args.cores, args.batch_size)
    return run_main(sso_genotype, sharded.sso_genotype_sharded, call, args)


def cli():
    run_cli(main)


if __name__ == "__main__":
    cli()

"""The one driver under `classic.sv_genotype` and `singlesample.sso_genotype`, and the one command line under their `main()`s.

`Driver.run` is the run both programs share: option checks, alignment files and native handles, libraries, the collector
for the chosen reader, device batches through `ChunkPipeline`, the bulk VCF route with its hand-over to the per-line
route, the `stats=` block.  What the reference's two programs do differently is NOT here: `classic.Classic` and
`singlesample.Sso` subclass `Driver` and state it, each piece with its `file:line` in the reference --

    data     flags, site_quals            the device pass
             count_mode                   how the reader counts towards max_reads
             qual_mode, bulk_under_debug  the bulk route
             skip_hash_lines              '#' lines in the body, on both routes
    methods  alignment_paths()            the names in `bam_string`, or the exit for one that is no *.bam / *.cram
             read_library_file(), write_library_file()
             open_vcf(bulk)               header in, header out, `self.fast`; the body as lines or as blocks of text
             warn(text), gather(sample, bp, max_reads)      inside handle_line
             render_actions(results, actions)               results -> the text of every output action
             finish(unpaired)             the end of a run
    data     alignment_outpath            (`svtyper -w`) the evidence dump: tag_and_write below, per chunk, in output order -- the reads of
                                                  reader="python", or the finished records of reader="device" (svt_dump_kernel.h)
             alignment_out                a writer that stands in for that BAM (bam.RecordSink: the sharded run, sharded.py)
             alignment_sort, alignment_index   (`--sort-alignment`, `--bai` / `--alignment-csi`) that BAM coordinate-sorted / with its .bai or .csi: the writer's
                                                  sort= and index= (bam.AlignmentFile), which hold the records until close()

No method takes a flag that names its caller, and a driver's hooks run per line handed to the per-line route and per
block, never per site of the bulk route (`BulkFeeder._block` / `_write_block`).
"""
from __future__ import annotations

import argparse
import os
import struct
import sys
from itertools import chain

from .bam import AlignmentFile, open_alignment_file
from .library import setup_sample
from .pipeline import (MIN_LIB_PREVALENCE, BulkFeeder, ChunkPipeline, NativeUnitCollector, UnitCollector, check_inflate,
                       check_cram, check_library_scan, check_verify, default_engine, resolve_reader, split_lines, verify_stats)
from .vcf import Variant, Vcf


# (breakpoint, sample) units per device batch of a run that writes the evidence dump (`svtyper -w`): every read object of a
# chunk stays alive until the chunk's verdicts are back, and ChunkPipeline keeps up to three chunks in flight.  A memory bound,
# not a measured optimum: 1 000 units of a few hundred reads each, a kilobyte or two per read object with its raw record, are a
# few hundred MB per chunk at the worst.
WRITE_CHUNK_UNITS = 1_000


def tag_and_write(evidence, out_bam, written: set) -> None:
    """The reads `svtyper -w` writes for the units of one chunk, tagged as the reference tags them (classic.py:296-413,
    parsers.py:771-782,1218-1228, utils.py:13-22).  `evidence`: per unit, in output order, None (a unit skipped by --max_reads, or
    one without reads) or (fragments, [packer.FragmentSpan], verdict bytes of the unit's records): is_ref_seq comes from the side
    table -- ungated, a hit with MAPQ 0 counts --, everything that depends on p_concordant, the small-deletion gate or a
    weight from the device (svt_batch_verdicts, bits 0-5).  `written`: the (query_name, flag) set of the whole run."""
    for unit in evidence:
        if unit is None:
            continue
        if not isinstance(unit, tuple):                         # the device reader's dump: the unit's reads as finished records, in that order
            _write_dumped(unit, out_bam, written)
            continue
        fragments, spans, verdicts = unit
        for span in spans:                                      # classic.py:296: sorted(query_name)
            fragment = fragments[span.name]
            first = int(verdicts[span.first])
            write_fragment = False
            for read, hit in zip(fragment.primary_reads, span.ref_hits):     # classic.py:306-314
                if hit:
                    read.set_tag("XV", "R")
                    write_fragment = True
            alt_split = set()                                   # classic.py:330: the candidates with p_alt > 0
            for k, split in enumerate(span.seq):
                if verdicts[span.first + k] & 16:
                    alt_split.add(id(split))
            for k, split in enumerate(span.clip):
                if verdicts[span.first + k] & 32:
                    alt_split.add(id(split))
            for split in fragment.split_reads:                  # classic.py:317-332
                if id(split) in alt_split:
                    split.read.set_tag("XV", "A")               # tag_split(p_alt > 0)
                    write_fragment = True
            if first & 1:                                       # classic.py:359-380: tag_span(p_alt)
                _tag_span(fragment, "A" if first & 2 else "R")
                write_fragment = True
            if first & 4:                                       # classic.py:398-408: tag_span(1 - p_conc)
                _tag_span(fragment, "A" if first & 8 else "R")
                write_fragment = True
            if write_fragment:                                  # classic.py:411-413
                for read in fragment.primary_reads + [split.read for split in fragment.split_reads]:
                    read.query_sequence = None                  # utils.py:13-22
                    key = (read.query_name, read.flag)
                    if key not in written:
                        out_bam.write(read)
                        written.add(key)


def open_alignment_writer(path, template_path, deflate, huffman, alignment_sort, alignment_index, device):
    """The `-w` BAM opened for writing, its header the template file's: with the run's compressor, and its order and index as the
    writer spells them (bam.AlignmentFile: sort=, index="bai", csi=True).  The one-process run opens it before its first record,
    the gathered run (sharded.py) on rank 0 once every rank's records are there."""
    if template_path.endswith(".cram"):     # (a CRAM's SAM header as a BAM holds it: cram.CramFile._header_bytes)
        from .cram import CramFile
        template = CramFile(template_path)
    else:
        template = AlignmentFile(template_path, "rb")
    order = dict(sort=True) if alignment_sort else {}
    if alignment_index is not None:         # (the writer spells a CSI as pysam does: the index asked for, csi=True)
        order["index"] = "bai"
        if alignment_index == "csi":
            order["csi"] = True
    try:
        return AlignmentFile(path, "wb", template=template, deflate=deflate, huffman=huffman, device=device, **order)
    finally:
        template.close()


def _write_dumped(records, out_bam, written: set) -> None:
    """A unit of the device reader's evidence dump (svt_dump_rules.h: tagged and cut as above, on the GPU): record by record, the
    key (query_name, flag) read at their fixed offsets, written unless the run wrote it before."""
    at, n = 0, len(records)
    while at < n:
        size = struct.unpack_from("<i", records, at)[0] + 4
        if size < 36 or at + size > n:
            raise ValueError("the evidence dump of a unit does not end with a whole record")
        l_read_name, flag = records[at + 12], struct.unpack_from("<H", records, at + 18)[0]
        key = (bytes(records[at + 36:at + 36 + l_read_name - 1]).decode("ascii"), flag)
        if key not in written:
            out_bam.write_raw(records[at:at + size])
            written.add(key)
        at += size


def _tag_span(fragment, value: str) -> None:
    """parsers.py:771-782: the primary reads that carry no XV yet"""
    for read in fragment.primary_reads:
        if not read.has_tag("XV"):
            read.set_tag("XV", value)


class Driver:
    flags = 0
    site_quals = False
    bulk_under_debug = True
    alignment_outpath = None            # (`svtyper -w`; classic.Classic sets it)
    deflate = "zlib"                    # who compresses the `-w` BAM's members (bam.BgzfWriter)
    huffman = "fixed"                   # ... and into which block, where it is the library's own compressor
    alignment_sort = False              # the `-w` BAM in coordinate order (bam.AlignmentFile: sort=)
    alignment_index = None              # ... and "bai" / "csi": its index beside it (index="bai"; "csi": with csi=True)
    cram_codec = None                   # "host" | "device": who decodes the rANS blocks of a CRAM among the inputs (None: the host twin)
    alignment_out = None                # a writer to use instead of opening alignment_outpath (write / write_raw / close: bam.RecordSink
                                        # under sharded.py); the run is then a `-w` run whether or not a path is given

    def __init__(self, bam_string, vcf_in, vcf_out, min_aligned, split_weight, disc_weight, num_samp, lib_info_path, debug,
                 ref_fasta, sum_quals, max_reads, max_ci_dist, n_threads=0):
        self.bam_string, self.vcf_in, self.vcf_out = bam_string, vcf_in, vcf_out
        self.min_aligned, self.split_weight, self.disc_weight = min_aligned, split_weight, disc_weight
        self.num_samp, self.lib_info_path, self.debug, self.ref_fasta = num_samp, lib_info_path, debug, ref_fasta
        self.sum_quals, self.max_reads, self.max_ci_dist = sum_quals, max_reads, max_ci_dist
        self.n_threads = n_threads      # of the C++ reader (0 = the library's default)
        self.fast = None                # SampleColumnWriter, made by open_vcf() once the header is known

    def run(self, chunk_units, engine=None, geometry="host", reader=None, stats=None, inflate="host", library_scan="host",
            verify="off"):
        writing = self.alignment_outpath is not None or self.alignment_out is not None
        reader = check_cram(self.bam_string, reader, inflate, library_scan, self.cram_codec)
        if not writing and (self.alignment_sort or self.alignment_index is not None):
            raise ValueError("alignment_sort / alignment_index (--sort-alignment, --bai) need -w/--write_alignment: they are about that BAM")
        if self.alignment_index not in (None, "bai", "csi"):
            raise ValueError("alignment_index must be None, 'bai' or 'csi', not %r" % (self.alignment_index,))
        if writing and reader is None:
            reader = "python"           # the one route that keeps the reads it tallied
        reader = resolve_reader(reader)
        if writing:
            self.check_write_alignment(reader, geometry, engine)
            chunk_units = min(chunk_units, WRITE_CHUNK_UNITS)
        check_inflate(reader, inflate)
        check_library_scan(reader, library_scan)
        verify_on = check_verify(verify)
        paths, bams = [], []
        for path in self.alignment_paths():
            paths.append(path)
            # (`-w` writes the records the built-in reader keeps the raw bytes of)
            bams.append(AlignmentFile(path, "rb", verify=verify_on) if writing and path.endswith(".bam")
                        else open_alignment_file(path, self.ref_fasta, verify=verify_on, cram_codec=self.cram_codec or "host",
                                                 device=getattr(engine, "device", 0)))
        lib_info = self.read_library_file()
        if self.vcf_in is None:     # classic.py:142-143 (sso_genotype does not get here without a VCF)
            sys.stderr.write("Warning: VCF not found.\n")
        native = None
        if reader in ("native", "device"):      # C++ reader: library scans now, fetch + fragment summaries later
            from .native_reads import NativeBam
            native = [NativeBam(p, verify=verify_on) for p in paths]
        if library_scan == "device" and lib_info is None and engine is None:
            engine = default_engine()               # (the scan runs on the device the pass will use)
        scan_device = getattr(engine, "device", 0) if library_scan == "device" else 0
        self.samples = [setup_sample(b, lib_info, self.num_samp, MIN_LIB_PREVALENCE, nb, library_scan, scan_device, inflate)
                        for b, nb in zip(bams, native or [None] * len(bams))]
        out_bam, written = None, set()
        if self.alignment_out is not None:
            out_bam = self.alignment_out
        elif writing:   # classic.py:161-166: the first alignment file is the template, its header is the dump's
            out_bam = open_alignment_writer(self.alignment_outpath, paths[0], self.deflate, self.huffman, self.alignment_sort,
                                            self.alignment_index, getattr(engine, "device", 0))
        self.write_library_file()
        if self.vcf_in is None:
            if out_bam is not None:     # classic.py:177-180
                out_bam.close()
            return
        try:
            self._run_body(chunk_units, engine, geometry, reader, stats, inflate, native, bams, out_bam, written)
        finally:
            if out_bam is not None:     # classic.py:527-531
                out_bam.close()

    @staticmethod
    def check_write_alignment(reader, geometry, engine):
        """`-w` needs the reads of a chunk alive when its verdicts come back, canonical records to give verdicts on, and an
        engine that gives them."""
        # reader="device" hands over the reads as finished records (the evidence dump) when the engine is the one whose batches the
        # device reader builds: the default engine, or one that declares supports_dump
        dumps = reader == "device" and (engine is None or getattr(engine, "supports_dump", False))
        if reader != "python" and not dumps:
            raise ValueError("-w/--write_alignment needs reader='python': reader=%r keeps no reads to write" % (reader,))
        if geometry == "device":
            raise ValueError("-w/--write_alignment needs geometry='host': with geometry='device' there are no canonical records on "
                             "the host to match the verdicts to")
        if engine is not None and not getattr(engine, "supports_verdicts", False):
            raise ValueError("-w/--write_alignment needs an engine with supports_verdicts (per-record verdicts beside the results)")

    def _run_body(self, chunk_units, engine, geometry, reader, stats, inflate, native, bams, out_bam, written):
        writing = out_bam is not None
        if engine is None:
            engine = default_engine()
        self.vcf = Vcf()
        if native is not None:      # C++ fetch + summariser; geometry in the reader's threads ("host") or on the device
            collector = NativeUnitCollector(self.samples, native, self.split_weight, self.disc_weight, self.min_aligned,
                                            self.count_mode, self.max_reads, n_threads=self.n_threads,
                                            geometry="walk" if reader == "device" else "device" if geometry == "device" else "reader",
                                            inflate=inflate, keep_reads=writing,
                                            gather=(lambda sample, bp, max_reads: self.gather(sample, bp, max_reads)) if writing else None)
        elif reader == "python":
            collector = UnitCollector(self.samples, self.split_weight, self.disc_weight, self.min_aligned, geometry,
                                      keep_reads=writing)
        else:
            raise ValueError("reader must be 'python', 'native' or 'device'")
        self.collector, self.native_sites = collector, native is not None
        pending: list = []      # ordered output actions of the current chunk
        pipe = ChunkPipeline()
        write = self.vcf_out.write

        def flush():
            actions = list(pending)
            pending.clear()
            # (classic) the incoming QUAL of every site: 0 unless --sum_quals
            quals = [float(a[1].qual) for a in actions if a[0] == "gt"] if self.site_quals else None
            pipe.submit(collector.take(engine, self.flags, site_quals=quals), lambda results: write_out(results, actions))

        def write_out(results, actions):
            if writing:
                tag_and_write(results.evidence, out_bam, written)
            for text in self.render_actions(results, actions):
                write(text)

        def per_line(lines):
            """the general route: one Variant object per line, device batches of `chunk_units` units"""
            for line in lines:
                if self.skip_hash_lines and line.startswith("#"):
                    continue
                action = self.handle_line(line)
                if action is not None:
                    pending.append(action)
                if len(collector) >= chunk_units:
                    flush()

        # bulk route (C++ reader): blocks of lines -> breakpoint arrays -> output text in native calls (bulk_vcf.py); lines it
        # hands back, and everything once it stops in front of a BND line it cannot express, take the per-line route above
        bulk = None
        # (under -w every line takes the per-line route: a unit the dump does not hold needs its breakpoint dict)
        if (native is not None and not writing and (self.bulk_under_debug or not self.debug) and hasattr(self.vcf_in, "read")
                and os.environ.get("SVT_BULK_VCF", "1") != "0"):
            from . import bulk_vcf
            if bulk_vcf.available():
                bulk = bulk_vcf
        lines, blocks = self.open_vcf(bulk is not None)
        feeder = rest = None
        if blocks is not None:
            feeder = BulkFeeder(bulk, self.vcf, collector, pipe, engine, self.flags, len(self.samples), self.fast, self.qual_mode,
                                self.max_ci_dist, self.sum_quals, self.skip_hash_lines, self.handle_line, self.render_actions, write)
            rest = feeder.run(blocks)
            if rest is not None:      # the per-line route from here on, with the BND mates the parser was holding
                for held in feeder.pending_lines():
                    mate = Variant(held.split("\t"), self.vcf)
                    if not self.sum_quals:
                        mate.qual = 0
                    self.vcf._bnd_pending[mate.var_id] = mate
                lines = chain(rest, chain.from_iterable(map(split_lines, blocks)))
        if lines is not None:
            per_line(lines)
        flush()
        pipe.close()
        if stats is not None:       # (keyword-only extra: where the caller's thread spent its time, pipeline.BulkFeeder.laps)
            stats.update(feeder.laps if feeder else {},
                         route="per line" if feeder is None else "bulk" if rest is None else "bulk, then per line")
            if reader == "device":      # the counters of svt_bam_evidence_device, summed over the run's calls
                stats["device_reader"] = collector.device_stats
            stats["verify"] = verify_stats(native, () if native else bams)   # (with the C++ reader the Python one reads the header only)
        # first BND mates whose partner never came: in the Vcf model, or left in the bulk parser at the end
        self.finish(bool(self.vcf._bnd_pending) or (feeder is not None and rest is None and feeder.n_pending() > 0))

    def handle_line(self, line, unit_base=0):
        """One variant line -> its output action (classic.py:213-278, singlesample.py:587-627), or None for a first BND
        mate (it waits for its partner in the Vcf model); its units go to the collector."""
        vcf, collector = self.vcf, self.collector
        var = Variant(line.rstrip().split("\t"), vcf)
        if not self.sum_quals:
            var.qual = 0
        if not var.has_svtype():
            self.warn("Warning: SVTYPE missing at variant %s. Skipping.\n" % var.var_id)
            return ("raw", var)
        if not var.is_valid_svtype():
            self.warn("Warning: Unsupported SVTYPE at variant %s (%s). Skipping.\n" % (var.var_id, var.get_svtype()))
            return ("raw", var)
        bp = vcf.get_variant_breakpoints(var, self.max_ci_dist)
        if bp is None:
            return None
        var2 = None
        if var.get_svtype() == "BND":       # the pair is written at the second mate's place, first mate first
            var2 = var
            var = vcf._bnd_first.pop(bp["id"])
        if self.native_sites:
            first_unit = collector.add_site(bp)
        else:
            first_unit = len(collector)
            for k, sample in enumerate(self.samples):
                fragments, many = self.gather(sample, bp, self.max_reads)
                collector.add(bp, k, fragments, skip=many)
        return ("gt", var, var2, first_unit - unit_base)


# ------------------------------------------------------------------------------------------ CLI
def parse_arguments(p, bam_help, max_reads, own):
    """The command line of `p` parsed: the arguments `svtyper` and `svtyper-sso` share, with `own(p)` adding a program's own
    where its help lists them."""
    p.add_argument("-i", "--input_vcf", metavar="FILE", type=argparse.FileType("r"), default=None,
                   help="VCF input (default: stdin)")
    p.add_argument("-o", "--output_vcf", metavar="FILE", type=argparse.FileType("w"), default=sys.stdout,
                   help="output VCF to write (default: stdout)")
    p.add_argument("-B", "--bam", metavar="FILE", type=str, required=True, help=bam_help)
    p.add_argument("-T", "--ref_fasta", metavar="FILE", type=str, default=None,
                   help="Indexed reference FASTA file (recommended for reading CRAM files)")
    p.add_argument("-S", "--split_bam", type=str, help=argparse.SUPPRESS)
    p.add_argument("-l", "--lib_info", metavar="FILE", dest="lib_info_path", type=str, default=None,
                   help="create/read JSON file of library information")
    p.add_argument("-m", "--min_aligned", metavar="INT", type=int, default=20,
                   help="minimum number of aligned bases to consider read as evidence [20]")
    p.add_argument("-n", dest="num_samp", metavar="INT", type=int, default=1000000,
                   help="number of reads to sample from BAM file for building insert size distribution [1000000]")
    p.add_argument("-q", "--sum_quals", action="store_true",
                   help="add genotyping quality to existing QUAL (default: overwrite QUAL field)")
    p.add_argument("--max_reads", metavar="INT", type=int, default=max_reads,
                   help="maximum number of reads to assess at any variant (default: %s)"
                        % ("unlimited" if max_reads is None else max_reads))
    p.add_argument("--max_ci_dist", metavar="INT", type=int, default=1e10,
                   help="maximum size of a confidence interval before 95%% CI is used intead (default: 1e10)")
    p.add_argument("--split_weight", metavar="FLOAT", type=float, default=1, help="weight for split reads [1]")
    p.add_argument("--disc_weight", metavar="FLOAT", type=float, default=1,
                   help="weight for discordant paired-end reads [1]")
    p.add_argument("--debug", action="store_true", help=argparse.SUPPRESS)
    own(p)
    # not in the reference: where the host work runs (same output bytes either way)
    p.add_argument("--reader", choices=("python", "native", "device"), default=None,
                   help="BAM access + fragment assembly: the C++ threads of libsvtyper_hip.so feeding the device "
                        "geometry stage, the same with the evidence records built on the GPU (device), or the portable Python "
                        "reader (same output bytes) [native]")
    p.add_argument("--inflate", choices=("host", "device"), default="host",
                   help="with --reader device: BGZF blocks inflated by the reader's threads, or on the GPU from the "
                        "compressed blocks (same output bytes) [host]")
    p.add_argument("--verify-bgzf", dest="verify_bgzf", action="store_true",
                   help="check the CRC32 of every BGZF block where it is inflated (verify='crc32'); a mismatch is an error")
    p.add_argument("--library-scan", dest="library_scan", choices=("host", "device"), default="host",
                   help="without a library file: the libraries' read length, insert-size histogram and prevalence from three "
                        "scans per library on the host, or from one segmented walk on the GPU for all libraries, members inflated as --inflate says "
                        "(needs --reader native or device; same library file, same output bytes) [host]")
    # (not listed by --help, like --bgzf: the help text is pinned byte for byte) who decodes the rANS blocks of a CRAM input
    p.add_argument("--cram-codec", dest="cram_codec", choices=("host", "device"), default=None, help=argparse.SUPPRESS)
    p.add_argument("--geometry", choices=("host", "device"), default="host",
                   help="with --reader python: breakpoint-dependent read predicates on the host or on the GPU [host]")
    add_output_arguments(p)
    args = p.parse_args()
    try:                        # the usage errors of a CRAM input (pipeline.check_cram)
        check_cram(args.bam, args.reader, args.inflate, args.library_scan, args.cram_codec)
    except ValueError as e:
        p.error(str(e))
    check_output_arguments(p, args, args.output_vcf)
    args.input_vcf = gzip_text(args.input_vcf)
    if args.input_vcf is None and not sys.stdin.isatty():
        args.input_vcf = sys.stdin
    return args


def add_output_arguments(p):
    """the options about the output file's format, of `svtyper`, `svtyper-sso` and `svtyper_amd.paste` alike"""
    # BGZF output (README).  Not listed by --help, like --debug: the help text of both programs is pinned byte for byte
    # (tests/golden/help_*.txt).  --bgzf: the output VCF as BGZF (.vcf.gz: what bcftools, tabix and IGV read); --deflate: who
    # compresses BGZF output (--bgzf, -w) -- zlib, or the library's own compressor on the host or on the GPU (same inflated bytes);
    # --huffman: the block that compressor writes -- fixed, or dynamic where that is shorter (not with --deflate zlib).
    # --sort: (with --bgzf) the body in stable order by (contig rank, POS); --tabix: (with --bgzf -o PATH) PATH.tbi beside the
    # output (bgzf_out's docstring: both hold the whole output text until the end); --csi: the same index in the CSI container,
    # PATH.csi, which also holds contigs beyond 512 Mbp (not together with --tabix).
    p.add_argument("--bgzf", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--deflate", choices=("zlib", "host", "device"), default="zlib", help=argparse.SUPPRESS)
    p.add_argument("--huffman", choices=("fixed", "dynamic"), default="fixed", help=argparse.SUPPRESS)
    p.add_argument("--sort", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--tabix", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--csi", action="store_true", help=argparse.SUPPRESS)
    # --bcf: the output as BCF2.2 in BGZF (bcf_out's docstring: what bcftools merge / concat / view -r read fastest); it takes
    # --sort, --csi (PATH.csi, the one index a BCF has), --deflate and --huffman, and neither --bgzf nor --tabix, which are about VCF text.
    p.add_argument("--bcf", action="store_true", help=argparse.SUPPRESS)


def check_output_arguments(p, args, output):
    """the usage errors of those options; `output`: the opened output file"""
    if args.bcf and args.bgzf:
        p.error("--bcf and --bgzf name two formats for one output: give one of them")
    if args.bcf and args.tabix:
        p.error("--tabix indexes VCF text: the index of a --bcf output is --csi")
    if (args.sort or args.tabix) and not (args.bgzf or args.bcf):
        p.error("--sort and --tabix need --bgzf")
    if args.csi and not (args.bgzf or args.bcf):
        p.error("--csi needs --bgzf")
    if args.csi and args.tabix:
        p.error("--csi and --tabix name two formats for one index: give one of them")
    if args.tabix and output is sys.stdout:
        p.error("--tabix needs an output file (-o): an index is written beside it")
    if args.csi and output is sys.stdout:
        p.error("--csi needs an output file (-o): an index is written beside it")


def gzip_text(vcf_in):
    """`-i PATH` whose first two bytes are 1f 8b (a .vcf.gz, BGZF or plain gzip): the file read through gzip as text.  Anything
    else, stdin included, as it is.  A BCF (BGZF whose payload begins with the BCF magic) is read as its VCF text, decoded by the
    host engine of bcf_in: a sites file is small."""
    path = getattr(vcf_in, "name", None)
    if vcf_in is None or vcf_in is sys.stdin or not isinstance(path, str) or not os.path.isfile(path):
        return vcf_in
    with open(path, "rb") as f:
        if f.read(2) != b"\x1f\x8b":
            return vcf_in
    from . import bcf_in
    if bcf_in.is_bcf(path):
        import io
        vcf_in.close()
        return io.TextIOWrapper(bcf_in.open_text(path, engine="host"))
    import gzip
    vcf_in.close()
    return gzip.open(path, "rt")


def run_main(driver, sharded_driver, call, args):
    """The tail of both `main()`s: `driver(*call)` with the options that are not in the reference -- or, launched by
    torch.distributed.run with several ranks, its sharded form: one GPU each, variants sharded, one gather."""
    from . import sharded
    if args.split_bam is not None:
        sys.stderr.write("Warning: --split_bam (-S) is deprecated. Ignoring %s.\n" % args.split_bam)
    options = dict(geometry=args.geometry, reader=check_cram(getattr(args, "bam", ""), args.reader) or "native", inflate=args.inflate, library_scan=args.library_scan,
                   verify="crc32" if args.verify_bgzf else "off")
    if getattr(args, "cram_codec", None) is not None:
        options["cram_codec"] = args.cram_codec
    job = sharded.job()
    if job is None:
        if not (args.bgzf or getattr(args, "bcf", False)):
            return driver(*call, **options)
        with _bgzf_text(call[2], args.deflate, 0, getattr(args, "huffman", "fixed"), args) as out:
            return driver(*call[:2], out, *call[3:], **options)
    rank, world, local_rank = job
    call = call[:2] + (sharded.private_stdout(call[2]),) + call[3:]
    engine = sharded.init(local_rank)
    if (args.bgzf or getattr(args, "bcf", False)) and rank == 0:             # (rank 0 writes everything: the others touch nothing)
        with _bgzf_text(call[2], args.deflate, getattr(engine, "device", local_rank), getattr(args, "huffman", "fixed"), args) as out:
            sharded_driver(*call[:2], out, *call[3:], rank=rank, world=world, engine=engine, **options)
    else:
        sharded_driver(*call, rank=rank, world=world, engine=engine, **options)
    sharded.finish()


def _bgzf_text(vcf_out, deflate, device, huffman="fixed", args=None):
    """`--bgzf`: the output VCF through bgzf_out.open_text; `--bcf`: through bcf_out.open_bcf (imported only here)"""
    if getattr(args, "bcf", False):
        from . import bcf_out
        return bcf_out.open_bcf(vcf_out, deflate=deflate, device=device, huffman=huffman, sort=bool(getattr(args, "sort", False)),
                                index="csi" if getattr(args, "csi", False) else None)
    from . import bgzf_out
    return bgzf_out.open_text(vcf_out, deflate=deflate, device=device, huffman=huffman, sort=bool(getattr(args, "sort", False)),
                              index="tbi" if getattr(args, "tabix", False) or getattr(args, "csi", False) else None,
                              csi=bool(getattr(args, "csi", False)))


def run_cli(main):
    try:
        sys.exit(main())
    except IOError as e:
        if e.errno != 32:   # EPIPE
            raise

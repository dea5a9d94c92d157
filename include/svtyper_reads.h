/*
 * svtyper_reads.h -- native (host, C++) BAM access + fragment summariser of libsvtyper_hip.so.
 *
 * The step BEFORE the device path: for every (breakpoint, sample) unit fetch the reads of the two
 * breakend regions from an indexed BAM, group them into read-fragments, run the
 * breakpoint-independent split-read QC and emit the fixed-size `svt_fragment` summaries
 * (include/svtyper_hip.h) that svt_batch_create_from_fragments consumes.  It replaces, for the
 * native pipeline, what the reference does with pysam objects in
 *   svtyper/classic.py:54-100   gather_all_reads / gather_reads            (count_mode 0)
 *   svtyper/singlesample.py:158-205  is_over_threshold / gather_reads      (count_mode 1)
 *   svtyper/parsers.py:729-768   SamFragment.__init__ / add_read
 *   svtyper/parsers.py:891-1058  SplitRead / SplitPiece / is_valid
 * and what svtyper_amd/bam.py + fragments.py + geometry.py do in Python (those stay the portable
 * implementation and are the checker of this one: tests/test_native_reads.py).
 *
 * Plain C ABI, host memory only; no GPU is needed for these calls.  BAM with a .bai or a .csi index.  (CRAM 3.0 is read by
 * svtyper_amd/cram.py on the Python reader route, over svt_rans_decode_* and svt_cram_decode_slice below; the svt_bam_* calls
 * take no CRAM.)
 */
#ifndef SVTYPER_READS_H
#define SVTYPER_READS_H

#include <stdint.h>

#include "svtyper_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svt_bam svt_bam; /* opaque: header + index of one BAM file */

/* Open `path` and its index: the first there is of `path`.bai, the .bai next to it, `path`.csi, the .csi next to it; the file's
 * magic, not its name, says whether it is a BAI or a CSI.  0 or SVT_ERR_*; text via svt_last_error(). */
int svt_bam_open(const char* path, svt_bam** out);
void svt_bam_close(svt_bam* bam);
/* Which index svt_bam_open took: *kind 1 for a BAI (min_shift 14, depth 5), 2 for a CSI with the scheme it names (positions
 * below 2^(min_shift + 3 * depth)); a null pointer is skipped.  Added under ABI 19 without a new number: a library built before
 * it lacks the symbol -- probe for it (dlsym / hasattr), as for svt_pack_evidence_flags. */
int svt_bam_index_info(const svt_bam* bam, int* kind, int* min_shift, int* depth);

int32_t svt_bam_n_references(const svt_bam* bam);
const char* svt_bam_reference_name(const svt_bam* bam, int32_t tid);
int64_t svt_bam_reference_length(const svt_bam* bam, int32_t tid);
int32_t svt_bam_tid(const svt_bam* bam, const char* name); /* -1 when absent */
/* the @RG / other header text (NUL-terminated), owned by the handle */
const char* svt_bam_header_text(const svt_bam* bam);

/* the two fetch windows of one unit (already clamped to the chromosome, pysam semantics:
 * reads with pos < hi and end > lo) */
typedef struct svt_fetch_unit {
    int32_t tid_a, lo_a, hi_a;
    int32_t tid_b, lo_b, hi_b;
} svt_fetch_unit;

typedef struct svt_summarise_args {
    uint64_t n_units;
    const svt_fetch_unit* windows;      /* n_units */
    const svt_breakpoint* breakpoints;  /* n_units: only pos_a / pos_b are read (interval choice) */
    uint32_t n_read_groups;
    const char* const* read_groups;     /* RG ids */
    const int32_t* read_group_lib;      /* library index of each RG; -1 = library not active
                                           (prevalence below the cut, classic.py:85-87)          */
    int64_t max_reads;                  /* < 0: unlimited                                         */
    int32_t count_mode;                 /* 0: classic.py:79-93 (position of the read in the fetch of
                                           one side > max_reads); 1: singlesample.py:158-185
                                           (bam.count() of either region > max_reads; counted
                                           while the reads are gathered, same outcome)           */
    int32_t n_threads;                  /* <= 0: all hardware threads                             */
} svt_summarise_args;

typedef struct svt_summaries {
    uint64_t* frag_offset;    /* n_units + 1 */
    svt_fragment* fragments;  /* frag_offset[n_units]; owned by the library (a large one comes from its pool of
                                 huge-page mappings): release ONLY through svt_summaries_free */
    uint8_t* skipped;         /* n_units: 1 = too many reads (unit has no fragments) */
} svt_summaries;

/* Summarise all units (multi-threaded over units; every thread has its own file handle).
 * On success the three arrays of `out` are owned by the caller: release with svt_summaries_free. */
int svt_bam_summarise(const svt_bam* bam, const svt_summarise_args* args, svt_summaries* out);
void svt_summaries_free(svt_summaries* s);

/* ---- the same units as evidence records ------------------------------------------------------
 * svt_bam_evidence = svt_bam_summarise + the breakpoint-dependent predicates of the geometry stage
 * (svtyper/parsers.py:785-857,1122-1215; what svt_batch_create_from_fragments evaluates on the
 * device) in the reader's own threads: 16-byte svt_records leave the reader instead of 128-byte
 * summaries, and the batch goes to svt_batch_create / svt_genotype like any other.  The predicates
 * are ONE piece of source for both places (svtyper_amd/csrc/svt_geometry_math.h); the records are
 * those of the device stage, byte for byte (tests/test_hip_geometry.py).
 * Here every field of svt_summarise_args.breakpoints is read.                                      */
typedef struct svt_evidence_params {
    uint32_t n_libs;           /* 1..65536: size of lib_flank; a fragment of a library beyond it is an error */
    const double* lib_flank;   /* per library: mean + 3 sd, is_pair_straddle's flank (parsers.py:846-855)   */
    int32_t min_aligned;       /* -m / --min_aligned (classic.py:34)                                        */
    int32_t split_slop;        /* 3 (classic.py:184)                                                        */
} svt_evidence_params;

typedef struct svt_evidence {
    uint64_t* rec_offset;     /* n_units + 1 */
    svt_record* records;      /* rec_offset[n_units], in the units' order, sorted(query_name) inside a unit;
                                 owned by the library: release ONLY through svt_evidence_free               */
    uint8_t* skipped;         /* n_units: 1 = too many reads (unit has no records; set SVT_UNIT_SKIP)       */
} svt_evidence;

int svt_bam_evidence(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out);
void svt_evidence_free(svt_evidence* e);

/* ---- the same records built from inflated BAM bytes by ONE piece of walk source (ABI 19) ---------
 * svtyper_amd/csrc/svt_evidence_walk.h restates decode / tag walk / split-read QC / fragment table of
 * the reader above as bounds-checked functions over bytes, compiled for the host and for the device.
 * It works inside a strict envelope (fixed capacities, well-formed records, known read groups); a unit
 * outside it is never guessed at: it is flagged with one of the reasons below.
 *
 * svt_bam_evidence_walk_host: the walk over host memory, no GPU, NO fallback -- a flagged unit comes
 * back empty with out_of_envelope[u] = its reason (0 = inside the envelope; a unit the max_reads rule
 * skips is `skipped`, not flagged).  For every unit that is not flagged rec_offset / records / skipped
 * are those of svt_bam_evidence, byte for byte.  `kept_reads` (n_units, may be null): reads the unit
 * keeps -- what SVT_WALK_CAP_READS bounds; the true number also for a unit flagged SVT_WALK_READS.
 * A unit of more than SVT_WALK_CAP_READS_LDS kept reads is walked by the deep tier of the same source
 * (tables from the heap, an O(n log^2 n) order).  Release `out` with svt_evidence_free.              */
#define SVT_WALK_RANGE 2       /* a record does not fit its range of inflated bytes (truncated / corrupt
                                  BGZF or record, record > 64 KiB, window on an unknown reference)      */
#define SVT_WALK_READS 3       /* more kept reads in the unit than SVT_WALK_CAP_READS                    */
#define SVT_WALK_NAME 4        /* query name longer than SVT_WALK_CAP_NAME                               */
#define SVT_WALK_CIGAR 5       /* more CIGAR operations (read or SA entry) than SVT_WALK_CAP_CIGAR       */
#define SVT_WALK_SA_CAP 6      /* SA value with more entries / bytes than SVT_WALK_CAP_SA_ENTRIES / _BYTES */
#define SVT_WALK_NO_RG 7       /* read without a usable RG tag                                           */
#define SVT_WALK_UNKNOWN_RG 8  /* RG not in the call's table, or its library beyond the library table    */
#define SVT_WALK_MALFORMED 9   /* malformed tag area, SA value or SA CIGAR                               */
#define SVT_WALK_MAPQ 10       /* SA MAPQ outside 0..255                                                 */
#define SVT_WALK_N_REASONS 11

#define SVT_WALK_CAP_READS 0        /* kept reads of a unit: the bound behind which it is flagged SVT_WALK_READS (16 384) */
#define SVT_WALK_CAP_NAME 1
#define SVT_WALK_CAP_CIGAR 2
#define SVT_WALK_CAP_SA_ENTRIES 3
#define SVT_WALK_CAP_SA_BYTES 4
#define SVT_WALK_CAP_RECORD 5
#define SVT_WALK_CAP_READS_LDS 6    /* kept reads up to which a unit's tables are on-chip (1 024); above: the deep tier    */
uint32_t svt_evidence_walk_capacity(int which);   /* SVT_WALK_CAP_*; 0 for an unknown one */

int svt_bam_evidence_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                               svt_evidence* out, uint8_t* out_of_envelope, uint32_t* kept_reads);

/* svt_bam_evidence_device: the reader stage with the walk on the GPU.  The host keeps the BAI lookup and the
 * BGZF inflate, uploads every inflated block once, one workgroup per unit builds the unit's records in HBM
 * (svt_evidence_kernel.h): units of up to SVT_WALK_CAP_READS_LDS kept reads with their tables in LDS, units of up
 * to SVT_WALK_CAP_READS kept reads by the deep kernel, whose tables are slices of an HBM workspace (at most 256 MiB,
 * allocated only by a call that has such units and released with it).  Every out-of-envelope unit is recomputed by
 * the host reader and spliced in, so the resident batch `*out` is the one svt_batch_create(svt_bam_evidence(...)) builds -- or the call fails with
 * the code and text svt_bam_evidence has for that unit.  `header`: n_units / units / n_libs / libs / weights of
 * the batch (rec_offset and records are ignored; SVT_UNIT_SKIP is set here for skipped units).  `skipped`
 * (n_units, may be null) and `stats` (may be null) are filled.  Needs a GPU.                               */
typedef struct svt_evidence_device_stats {
    uint64_t n_units;
    uint64_t reads_walked;                          /* records in the units' ranges                         */
    uint64_t units_skipped;
    uint64_t units_host;                            /* recomputed by the host reader ...                    */
    uint64_t units_host_by_reason[SVT_WALK_N_REASONS]; /* ... by SVT_WALK_* reason                          */
    uint64_t n_records;
    uint64_t bytes_uploaded;                        /* arena + ranges + unit arrays                         */
    double host_arena_s;                            /* BAI lookup + inflate + arena                         */
    double upload_s;
    double device_walk_s;                           /* the two launches, host-observed                      */
    double host_fallback_s;
    double batch_create_s;
} svt_evidence_device_stats;

int svt_bam_evidence_device(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                            const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out,
                            uint8_t* skipped, svt_evidence_device_stats* stats);

/* The deep tier's share of the calling thread's most recent svt_bam_evidence_device / _device_inflate call
 * (thread-local, as svt_last_error's text; zeros before the first call and for a call without deep units).  */
typedef struct svt_evidence_deep_stats {
    uint64_t units_deep;        /* units walked by the deep kernel      */
    uint64_t reads_deep;        /* kept reads of those units            */
    uint64_t workspace_bytes;   /* size of the HBM slab                 */
    double   deep_walk_s;       /* both deep launches, host-observed    */
} svt_evidence_deep_stats;
int svt_evidence_device_deep_stats(svt_evidence_deep_stats* out);

/* ---- BGZF inflate by ONE piece of decoder source, and the device reader that uses it (additions to ABI 19) ----
 * svtyper_amd/csrc/svt_inflate.h decodes the raw-deflate payload of a BGZF member (stored, fixed and dynamic blocks)
 * into exactly ISIZE bytes or a status; it is compiled for the host and for the device (svt_inflate_kernel.h, one
 * wavefront per member).  The verdict is the host reader's and zlib's: the stream ends with its final block having
 * produced exactly ISIZE bytes; bytes behind the final block are ignored.  The trailer's CRC32 is checked under verify only
 * (the _verified entry points and svt_bam_set_verify below), by svtyper_amd/csrc/svt_crc32.h.
 *
 * svt_bgzf_inflate_host / _device: `data[len]` holds whole BGZF members at block_off[0..n); member k goes to
 * out + out_off[k] and has to fill out_off[k + 1] - out_off[k] bytes (the caller's prefix sums of ISIZE).
 * status[k]: 0 or an SVT_INFLATE_* reason; the bytes of a failed member are undefined.  The return value is
 * about the arguments (and the GPU), not about the members.                                                  */
#define SVT_INFLATE_INPUT 1     /* the payload ends inside the stream                                         */
#define SVT_INFLATE_BTYPE 2     /* block type 3                                                               */
#define SVT_INFLATE_STORED 3    /* stored block: LEN / NLEN disagree                                          */
#define SVT_INFLATE_LENGTHS 4   /* bad code-length set (over- / under-subscribed, bad repeat, no end-of-block)*/
#define SVT_INFLATE_SYMBOL 5    /* bits that are no code / literal-length symbol 286, 287                     */
#define SVT_INFLATE_DISTANCE 6  /* distance symbol 30, 31 / distance before the start of the output           */
#define SVT_INFLATE_OUTPUT 7    /* more than ISIZE bytes                                                      */
#define SVT_INFLATE_SHORT 8     /* the stream ends with fewer than ISIZE bytes                                */
#define SVT_INFLATE_MEMBER 9    /* no BGZF member at the offset / ISIZE is not the place it was given         */
int svt_bgzf_inflate_host(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                          const uint64_t* out_off, uint32_t* status);
int svt_bgzf_inflate_device(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                            const uint64_t* out_off, uint32_t* status, int device);

/* ---- the CRC-32 of BGZF members, by ONE piece of source on the host and on the device (additions to ABI 19) ----
 * svtyper_amd/csrc/svt_crc32.h computes the CRC-32 of gzip over a member's inflated bytes: 64 chunks on 16-byte
 * boundaries, a table-driven CRC per chunk, the registers joined by multiplications mod P (svt_crc32_kernel.h: one
 * wavefront per member, one lane per chunk; on the host one loop over the chunks).
 *
 * svt_bgzf_crc32_host / _device: member k is bytes[off[k] .. off[k + 1]) -- off holds n + 1 non-decreasing offsets,
 * a member has at most 65 536 bytes --, crc[k] receives its CRC-32.  Host memory for the one; for the other `bytes`
 * is a pointer into the memory of `device` (off and crc are host arrays).
 *
 * svt_bgzf_inflate_host_verified / _device_verified: svt_bgzf_inflate_host / _device, and a member that inflates
 * but whose CRC-32 is not the one its trailer stores gets SVT_INFLATE_CRC.  The decode verdict comes first: a member
 * with another status keeps it.                                                                                */
#define SVT_INFLATE_CRC 10      /* inflated to ISIZE bytes whose CRC-32 is not the trailer's (verify only)       */
int svt_bgzf_crc32_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t* crc);
int svt_bgzf_crc32_device(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t* crc, int device);
int svt_bgzf_inflate_host_verified(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                   const uint64_t* out_off, uint32_t* status);
int svt_bgzf_inflate_device_verified(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                     const uint64_t* out_off, uint32_t* status, int device);

/* ---- BGZF deflate by ONE piece of source (additions; the ABI number stays: probe for the symbols) ------------------
 * svtyper_amd/csrc/svt_deflate.h compresses the payload of a BGZF member, 0 .. 65 280 bytes, into one fixed-Huffman
 * (or stored) block whose bytes are a function of the payload alone: 64 chunks, a greedy parse per
 * chunk over a private table seeded with the chunk in front.  It is compiled for the host and for the device
 * (svt_deflate_kernel.h, one wavefront per member); both write the same bytes.
 *
 * Payload k is bytes[off[k] .. off[k + 1]) -- off holds n + 1 non-decreasing offsets.  Whole members (the header
 * bam.BgzfWriter writes, the deflate bytes, the CRC-32 by svt_crc32.h, ISIZE) land side by side in out[0, capacity)
 * at out_off[0 .. n] (out_off holds n + 1 entries, out_off[0] = 0).  All arrays are host memory.  SVT_ERR_INVALID:
 * a payload above 65 280 bytes, offsets that decrease, a capacity below what the members need (out is never
 * overrun; payload bytes + 31 n always suffice).                                                                    */
int svt_bgzf_deflate_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity,
                          uint64_t* out_off);
int svt_bgzf_deflate_device(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity,
                            uint64_t* out_off, int device);
/* the calling thread's most recent svt_bgzf_deflate_device: its kernels by HIP events, apart from the copies */
typedef struct svt_deflate_times {
    double crc_kernel_s, deflate_kernel_s, pack_kernel_s;
    double total_s;             /* the whole call on the host's clock: upload, kernels, download                     */
} svt_deflate_times;
int svt_bgzf_deflate_last_times(svt_deflate_times* times);

/* The block a member is written as (additions; probe for the symbols).  SVT_DEFLATE_FIXED: the two entries above, byte
 * for byte.  SVT_DEFLATE_DYNAMIC: the same tokens in one dynamic-Huffman block whose code is made from the member's own
 * token histogram, wherever that block is strictly shorter than what SVT_DEFLATE_FIXED writes for the
 * member, and exactly those bytes otherwise -- so no member grows and every capacity rule above holds unchanged.  Host
 * and device write the same bytes.  Any other mode: SVT_ERR_INVALID.  svt_bgzf_deflate_last_times answers for the
 * calling thread's last device call of either kind.                                                                 */
#define SVT_DEFLATE_FIXED 0u
#define SVT_DEFLATE_DYNAMIC 1u
int svt_bgzf_deflate_host_mode(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity,
                               uint64_t* out_off, uint32_t mode);
int svt_bgzf_deflate_device_mode(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity,
                                 uint64_t* out_off, uint32_t mode, int device);
/* The code-length rule of the dynamic block on its own (the seam svt_bayes_gt is for the likelihoods): `sets`
 * histograms of `symbols` frequencies each, side by side in freq, -> their code lengths of at most `limit` bits, side
 * by side in lengths (0: the symbol has no code).  Huffman's optimum wherever that fits the limit, complete and never
 * over-subscribed otherwise; one used symbol gets one bit, none no code.  On the device one wavefront per histogram,
 * through the compressor's own source.  SVT_ERR_INVALID: limit other than 7 or 15, symbols outside 1 .. 286, a
 * histogram whose frequencies sum to 2^32 or more or that uses more than 2^limit symbols.                           */
int svt_huffman_lengths_host(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, uint8_t* lengths);
int svt_huffman_lengths_device(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, uint8_t* lengths,
                               int device);

/* ---- VCF text as lines: sorted, tabix-indexed BGZF output (additions; the ABI number stays: probe for the symbols) ----
 * svtyper_amd/csrc/svt_vcf_lines.h holds the per-line rule of the tabix VCF preset as one piece of
 * source for the host and the device (svt_vcf_lines_kernel.h).  A line is the bytes up to and including '\n'; the last
 * one may lack it.  One record per line, in text order:
 *   off, len     where the line lies in the text and how long it is (its newline included)
 *   flags        SVT_TBX_META: it starts with '#'.  SVT_TBX_BAD: not a data line (fewer than 8 tab-separated columns, a
 *                POS that is not 1 .. 10 decimal digits below 2^31, an empty line).  SVT_TBX_RANGE: end > 2^29, beyond
 *                what a TBI index addresses (a CSI index holds it: svt_csi_build_vcf).
 *   beg, end     (data lines) beg = max(POS - 1, 0); end = beg + len(REF), or the value of the first INFO key END (at the
 *                start of INFO or behind ';', followed by '=' and a digit) where it has at most 10 digits and lies above
 *                beg; saturated at 2^32 - 1
 *   chrom_len    bytes of the CHROM column                                                                            */
typedef struct svt_tbx_line {
    uint64_t off, len;
    uint32_t beg, end, chrom_len, flags;
} svt_tbx_line;
#define SVT_TBX_META 1u
#define SVT_TBX_BAD 2u
#define SVT_TBX_RANGE 4u
/* what a body line cannot be for svt_vcf_sort_order / svt_tbx_build (bad_kind) */
#define SVT_TBX_NOT_DATA 1u      /* a '#' line behind the first data line, or a SVT_TBX_BAD one                        */
#define SVT_TBX_BEYOND 2u        /* SVT_TBX_RANGE                                                                      */
#define SVT_TBX_CONTIG_AGAIN 3u  /* a contig that reappears behind another one                                         */
#define SVT_TBX_POS_BACK 4u      /* beg below the beg of the line in front, on the same contig                         */
/* The line table of text[0, len): lines[0, *n_lines).  SVT_ERR_INVALID where capacity is below the number of lines
 * (*n_lines is set all the same; the newlines of the text and one always suffice).                                  */
int svt_vcf_lines_host(const uint8_t* text, uint64_t len, svt_tbx_line* lines, uint64_t capacity, uint64_t* n_lines);
int svt_vcf_lines_device(const uint8_t* text, uint64_t len, svt_tbx_line* lines, uint64_t capacity, uint64_t* n_lines,
                         int device);
/* Line lines[perm[j]] of the text becomes line j of out[0, out_len): out_len is the sum of their lengths.            */
int svt_vcf_gather_host(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm,
                        uint64_t n_perm, uint8_t* out, uint64_t out_len);
int svt_vcf_gather_device(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm,
                          uint64_t n_perm, uint8_t* out, uint64_t out_len, int device);
/* The order --sort writes: the header (the '#' lines in front of the first other line) as it is, then the body in
 * stable order by (contig rank, POS): the rank of a contig is its place among the header's ##contig=<ID=...> lines,
 * the contigs the header does not declare behind them in order of first appearance.  perm holds n entries.  A body
 * line that is no data line: *bad_line is its 1-based number (SVT_OK, perm undefined); 0 otherwise.                 */
int svt_vcf_sort_order(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, uint64_t* perm,
                       uint64_t* bad_line);
/* One call for the writer with deflate="device": the text goes up once; its line table is made there; with sort != 0
 * the keys come down, the order goes up and the lines are gathered into a second buffer; the text as written is cut
 * every 65 280 bytes and compressed by the kernels of svt_bgzf_deflate_device_mode (the same members, byte for
 * byte).  out / capacity / out_off (ceil(len / 65280) + 1 entries) as there.  lines[0, *n_lines): the table of the
 * text as written; src_off[j]: where written line j lies in the caller's text.  *bad_line as svt_vcf_sort_order
 * (then nothing is compressed).                                                                                      */
int svt_vcf_bgzf_device(const uint8_t* text, uint64_t len, int sort, uint32_t mode, uint8_t* out, uint64_t capacity,
                        uint64_t* out_off, svt_tbx_line* lines, uint64_t line_capacity, uint64_t* n_lines,
                        uint64_t* src_off, uint64_t* bad_line, int device);
/* the calling thread's most recent svt_vcf_lines_device / _gather_device / _bgzf_device: its kernels by HIP events */
typedef struct svt_vcf_lines_times {
    double count_kernel_s, starts_kernel_s, parse_kernel_s, gather_kernel_s;
    double total_s;             /* the whole call on the host's clock                                                */
} svt_vcf_lines_times;
int svt_vcf_lines_last_times(svt_vcf_lines_times* times);
/* Per-sample VCFs joined by line number (svtyper_amd/paste.py; the reference's scripts/vcf_paste.py, and with
 * SVT_PASTE_AFREQ its scripts/vcf_allele_freq.py behind it).  Added without a new SVT_ABI_VERSION: probe for the symbol.
 * One call takes one block: text[0, len) holds n_lines body lines of the master and of each of the n_inputs inputs, every
 * line with its newline; file f's line j is line first_line[f] + j of the text (file 0: the master, f: input f - 1).
 * info_table (SVT_PASTE_AFREQ): the output header's INFO ids in its order, "V<id>\n" each, "F<id>\n" for a Flag.
 * results[0, n_lines): one record per output line:
 *   qual         the master's QUAL and every input's, added in file order
 *   counts       (SVT_PASTE_AFREQ) how often allele 0 .. 7 stands in a GT; nonref: the GTs with a non-reference allele
 *   flags        SVT_PASTE_SLOW_*: why the line was left to the plain C++ of the host (a QUAL outside the exact float
 *                rule, fewer than nine columns, a GT that is not digits joined by one separator or has more than eight
 *                alleles, an allele index above the ALT count, more than seven ALTs); SVT_PASTE_UNSAFE: SVT_PASTE_SAFE
 *                found CHROM, POS or ID (bad_field 0, 1, 2) of input bad_input to differ from the master's
 *   part_len     the inputs' sample columns with a tab in front of each input's; line_len: the output line
 * out[0, info->out_len): the block's output lines.  A line that cannot be written: info->bad_line is its 1-based number in
 * the block, bad_file the file (as above), bad_kind SVT_PASTE_BAD_*, and nothing is written (SVT_OK all the same).
 * SVT_ERR_INVALID where capacity is below the output.  svt_vcf_paste_device: the same bytes and results from the two
 * kernels of svt_vcf_paste_kernel.h; bits 8-9 of flags choose how the write kernel spreads its lanes over the sample
 * parts (0: the default, 1: a lane, 2: a quarter of the wavefront, 3: the wavefront per part).                        */
typedef struct svt_paste_line {
    double qual;
    uint32_t counts[8];
    uint32_t nonref, flags, bad_input, bad_field, part_len, line_len;
} svt_paste_line;
typedef struct svt_paste_info {
    uint64_t out_len, host_lines, bad_line;
    uint32_t bad_file, bad_kind, bad_field, reserved;
} svt_paste_info;
#define SVT_PASTE_SUM_QUALS 1u
#define SVT_PASTE_AFREQ 2u
#define SVT_PASTE_SAFE 4u
#define SVT_PASTE_LAYOUT_SHIFT 8
#define SVT_PASTE_SLOW_QUAL 1u
#define SVT_PASTE_SLOW_COLUMNS 2u
#define SVT_PASTE_SLOW_GT 4u
#define SVT_PASTE_SLOW_ALLELE 8u
#define SVT_PASTE_SLOW_ALT 16u
#define SVT_PASTE_UNSAFE 32u
#define SVT_PASTE_BAD_QUAL 1u     /* a QUAL that float() refuses                                                        */
#define SVT_PASTE_BAD_COLUMNS 2u  /* a line without the column the scripts index                                        */
#define SVT_PASTE_BAD_GT 3u       /* a GT whose alleles int() refuses                                                   */
#define SVT_PASTE_BAD_ALLELE 4u   /* an allele index beyond the ALT count                                               */
#define SVT_PASTE_BAD_POS 5u      /* (SVT_PASTE_AFREQ) a POS that int() refuses                                         */
#define SVT_PASTE_BAD_UNSAFE 6u   /* SVT_PASTE_SAFE: bad_field of bad_file differs from the master's                    */
int svt_vcf_paste_host(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines,
                       uint32_t flags, const uint8_t* info_table, uint64_t info_len, uint8_t* out, uint64_t capacity,
                       svt_paste_line* results, svt_paste_info* info);
int svt_vcf_paste_device(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines,
                         uint32_t flags, const uint8_t* info_table, uint64_t info_len, uint8_t* out, uint64_t capacity,
                         svt_paste_line* results, svt_paste_info* info, int device);
/* the calling thread's most recent svt_vcf_paste_device: its kernels by HIP events, its copies on the host's clock    */
typedef struct svt_vcf_paste_times {
    double lines_kernels_s, measure_kernel_s, write_kernel_s;
    double upload_s, download_s, host_s;   /* the text up; the results and the pasted text down; the lines' first columns */
    double total_s;
} svt_vcf_paste_times;
int svt_vcf_paste_last_times(svt_vcf_paste_times* times);
/* The read-depth classifier of DEL and DUP lines (svtyper_amd/classify.py; the reference's scripts/sv_classifier.py).
 * Added without a new SVT_ABI_VERSION: probe for the symbol.  One call takes one block: text[0, len) holds body lines of the
 * cohort VCF, every line with its newline, each with n_samples sample columns.  male, female, excluded [n_samples]: one
 * byte per sample of the header, 1 where the gender file says 1 (male) or 2 (female) and where the exclude file names
 * the sample; a sample the gender file does not name is SVT_CLASSIFY_NO_GENDER in male and in female.  format_table: the
 * output header's FORMAT ids in its order ("GT\n" first), "<id>\n" each.  skip [n_lines] or NULL: 1 for a line the
 * caller has settled already (an MEI): its record is route SVT_CLASSIFY_SKIPPED and nothing else is looked at.
 * results[0, *n_lines), capacity records: one per line of the text:
 *   route        SVT_CLASSIFY_VERBATIM (the first INFO item "SVTYPE=" is not DEL or DUP: the line is written as it is),
 *                _LOW (fewer than 10 positive samples: medians), _HIGH (the regression), _DROPPED (a later SVTYPE item
 *                is neither: the script writes nothing), _SKIPPED
 *   verdict      1: read depth supports the call, the line stays; 0: it is split into two BND lines
 *   n_pos        the samples not excluded whose GT is neither "./." nor "0/0"
 *   n_ref, n_alt (low) the two lists of CN values the script compares; quorum: the supporting ones of n_alt;
 *                median, mad: of the n_ref values (0 where there is none)
 *   slope, r2, n_regressed   (high) of CN against AB over the samples whose AB is neither "." nor -1 (0 where the
 *                regression does not run: no CN, a uniform AB or CN)
 *   flags        SVT_CLASSIFY_SLOW_*: why the line was left to the plain C++ of the host (values and verdict are then
 *                that code's); SVT_CLASSIFY_NEAR: r2 or the signed slope lies within 1e-9 (relative; absolute for a
 *                threshold of 0) of its threshold; SVT_CLASSIFY_DEL: the type is DEL
 * A line the script dies on: info->bad_line is its 1-based number in the block, bad_kind SVT_CLASSIFY_BAD_*, bad_sample
 * the sample (or 0xFFFFFFFF), bad_text the key or token in the way (SVT_OK all the same).  svt_vcf_classify_device: the
 * same records from svt_vcf_classify_kernel.h, byte for byte.
 * svt_vcf_classify_write: the output text of the block from its records (both engines' text is written here): verbatim
 * lines as they are, kept lines rebuilt as get_var_string does, the others as their two BND lines; out_off[0 .. n_lines]
 * is where each line's output lies (skipped and dropped lines: nothing).  The text is kept for the calling thread:
 * info->out_len is its length, svt_vcf_classify_take copies it out.  info_table: as svt_vcf_paste_host's.               */
typedef struct svt_classify_line {
    double median, mad, slope, r2;
    uint32_t route, verdict, n_pos, n_ref, n_alt, quorum, n_regressed, flags;
} svt_classify_line;
typedef struct svt_classify_info {
    uint64_t out_len, host_lines, near_lines, bad_line;
    uint32_t bad_kind, bad_sample;
    char bad_text[48];
} svt_classify_info;
#define SVT_CLASSIFY_CAPACITY 4096u  /* the samples of a line the kernel holds in LDS                                  */
#define SVT_CLASSIFY_NO_GENDER 255u
#define SVT_CLASSIFY_VERBATIM 0u
#define SVT_CLASSIFY_LOW 1u
#define SVT_CLASSIFY_HIGH 2u
#define SVT_CLASSIFY_DROPPED 3u
#define SVT_CLASSIFY_SKIPPED 4u
#define SVT_CLASSIFY_SLOW_HEAD 1u      /* fewer than ten columns, a POS or QUAL outside the exact rules, SVTYPE twice   */
#define SVT_CLASSIFY_SLOW_FORMAT 2u    /* FORMAT is not GT first and the header's keys in the header's order           */
#define SVT_CLASSIFY_SLOW_COLUMNS 4u   /* not one column per sample of the header                                       */
#define SVT_CLASSIFY_SLOW_SAMPLE 8u    /* a sample column without exactly FORMAT's fields                               */
#define SVT_CLASSIFY_SLOW_TOKEN 16u    /* a CN or AB outside bcf::double_exact                                          */
#define SVT_CLASSIFY_SLOW_CAPACITY 32u /* more than SVT_CLASSIFY_CAPACITY samples, or none                              */
#define SVT_CLASSIFY_SLOW_GENDER 64u   /* X or Y and a sample without a gender                                          */
#define SVT_CLASSIFY_SLOW_KEYS 128u    /* the route reads a CN or AB that FORMAT lacks                                  */
#define SVT_CLASSIFY_SLOW 255u
#define SVT_CLASSIFY_NEAR 256u
#define SVT_CLASSIFY_DEL 512u
#define SVT_CLASSIFY_BAD_COLUMNS 1u    /* fewer than eight columns (IndexError)                                         */
#define SVT_CLASSIFY_BAD_POS 2u        /* a POS that int() refuses (ValueError)                                         */
#define SVT_CLASSIFY_BAD_QUAL 3u       /* a QUAL that float() refuses (ValueError)                                      */
#define SVT_CLASSIFY_BAD_FORMAT 4u     /* a FORMAT key the header does not declare (the script's message, status 1)     */
#define SVT_CLASSIFY_BAD_KEY 5u        /* bad_text: the FORMAT key a sample or the INFO key the line lacks (KeyError)   */
#define SVT_CLASSIFY_BAD_NUMBER 6u     /* bad_text: a CN or AB that float() refuses (ValueError)                        */
#define SVT_CLASSIFY_BAD_NONFINITE 7u  /* bad_text: a CN or AB that is nan or inf (a departure: DESIGN 3.4)             */
#define SVT_CLASSIFY_BAD_GENDER 8u     /* X or Y and a sample the gender file does not name (KeyError)                  */
int svt_vcf_classify_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                          const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip,
                          double slope_threshold, double rsquared_threshold, svt_classify_line* results, uint64_t capacity,
                          uint64_t* n_lines, svt_classify_info* info);
int svt_vcf_classify_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                            const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip,
                            double slope_threshold, double rsquared_threshold, svt_classify_line* results, uint64_t capacity,
                            uint64_t* n_lines, svt_classify_info* info, int device);
int svt_vcf_classify_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                           const uint8_t* format_table, uint64_t format_len, const svt_classify_line* results, uint64_t n_lines,
                           uint64_t* out_off, svt_classify_info* info);
int svt_vcf_classify_take(uint8_t* out, uint64_t capacity);
/* the calling thread's most recent svt_vcf_classify_device: its kernels by HIP events, its copies on the host's clock  */
typedef struct svt_vcf_classify_times {
    double lines_kernels_s, classify_kernel_s;
    double upload_s, download_s, host_s;    /* the text up; the records down; the marked lines on the host             */
    double total_s;
} svt_vcf_classify_times;
int svt_vcf_classify_last_times(svt_vcf_classify_times* times);
/* PE, SR, SU and MSQ of a cohort VCF from the genotyper's evidence (svtyper_amd/update_info.py; the reference's
 * scripts/update_info.py).  Added without a new SVT_ABI_VERSION: probe for the symbol.  One call takes one block, as
 * svt_vcf_classify_host does: text[0, len) holds body lines, every line with its newline; format_table: the output
 * header's FORMAT ids in its order ("GT\n" first), "<id>\n" each.  results[0, *n_lines), capacity records, one per line:
 *   pe, sr       int(AP) and int(AS) added over the header's samples
 *   sum_sq       the bits of the double that float(SQ) of the positive samples (GT neither "0/0" nor "./.") add up to, in
 *                sample order from +0.0; num_pos: how many they are
 *   route        SVT_UPDATE_INFO_RULE: the per-line rule computed the record and the sample part of the output is a slice
 *                of the input; _PLAIN: the plain C++ of the host did, and the line is written again field by field
 *   flags        SVT_UPDATE_INFO_SLOW_*: why the line was left to the plain C++
 * A line the script dies on: info->bad_line is its 1-based number in the block, bad_kind SVT_UPDATE_INFO_BAD_*, bad_sample
 * the sample (or 0xFFFFFFFF), bad_text the key or token in the way (SVT_OK all the same).  svt_vcf_update_info_device: the
 * same records from svt_vcf_update_info_kernel.h, byte for byte.
 * svt_vcf_update_info_write: the output text of the block from its records (both engines' text is written here), every
 * line rebuilt as the script's get_var_string does with PE, SR, SU and MSQ set; out_off[0 .. n_lines] is where each line's
 * output lies.  info_table: as svt_vcf_paste_host's, without SNAME and with MSQ.  The text is kept for the calling thread:
 * info->out_len is its length, svt_vcf_update_info_take copies it out.                                                  */
typedef struct svt_update_info_line {
    int64_t pe, sr;
    uint64_t sum_sq;
    uint32_t num_pos, route, flags, reserved;
} svt_update_info_line;
typedef struct svt_update_info_report {
    uint64_t out_len, host_lines, bad_line;
    uint32_t bad_kind, bad_sample;
    char bad_text[48];
} svt_update_info_report;
#define SVT_UPDATE_INFO_CAPACITY 4096u    /* the samples of a line the kernel holds in LDS                              */
#define SVT_UPDATE_INFO_RULE 0u
#define SVT_UPDATE_INFO_PLAIN 1u
#define SVT_UPDATE_INFO_SLOW_HEAD 1u      /* fewer than nine columns, a POS or QUAL outside the exact rules              */
#define SVT_UPDATE_INFO_SLOW_FORMAT 2u    /* FORMAT is not GT first and the header's keys in the header's order         */
#define SVT_UPDATE_INFO_SLOW_COLUMNS 4u   /* not one column per sample of the header                                     */
#define SVT_UPDATE_INFO_SLOW_SAMPLE 8u    /* a sample column without exactly FORMAT's fields                             */
#define SVT_UPDATE_INFO_SLOW_TOKEN 16u    /* an AP or AS that is not one to nine digits, an SQ outside bcf::double_exact  */
#define SVT_UPDATE_INFO_SLOW_CAPACITY 32u /* more than SVT_UPDATE_INFO_CAPACITY samples, or none                         */
#define SVT_UPDATE_INFO_SLOW_KEYS 64u     /* FORMAT lacks AP or AS, or SQ where a sample is positive                     */
#define SVT_UPDATE_INFO_SLOW 127u
#define SVT_UPDATE_INFO_BAD_COLUMNS 1u    /* fewer than seven columns (IndexError)                                       */
#define SVT_UPDATE_INFO_BAD_POS 2u        /* a POS that int() refuses (ValueError)                                       */
#define SVT_UPDATE_INFO_BAD_QUAL 3u       /* a QUAL that float() refuses (ValueError)                                    */
#define SVT_UPDATE_INFO_BAD_FORMAT 4u     /* a FORMAT key the header does not declare (the script's message, status 1)   */
#define SVT_UPDATE_INFO_BAD_KEY 5u        /* bad_text: the FORMAT key the sample lacks (KeyError)                        */
#define SVT_UPDATE_INFO_BAD_NUMBER 6u     /* bad_text: an AP, AS or SQ that int() or float() refuses (ValueError)        */
#define SVT_UPDATE_INFO_BAD_NONFINITE 7u  /* bad_text: an SQ that is nan or inf (a departure: DESIGN 3.4)                */
#define SVT_UPDATE_INFO_BAD_OVERFLOW 8u   /* a count or a sum beyond int64 (a departure: DESIGN 3.4)                     */
#define SVT_UPDATE_INFO_BAD_EIGHT 9u      /* seven columns (the script's message, status 1)                              */
int svt_vcf_update_info_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                             svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines, svt_update_info_report* info);
int svt_vcf_update_info_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table,
                               uint64_t format_len, svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines,
                               svt_update_info_report* info, int device);
int svt_vcf_update_info_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                              const uint8_t* format_table, uint64_t format_len, const svt_update_info_line* results,
                              uint64_t n_lines, uint64_t* out_off, svt_update_info_report* info);
int svt_vcf_update_info_take(uint8_t* out, uint64_t capacity);
/* the calling thread's most recent svt_vcf_update_info_device: its kernels by HIP events, its copies on the host's clock */
typedef struct svt_vcf_update_info_times {
    double lines_kernels_s, update_info_kernel_s;
    double upload_s, download_s, host_s;    /* the text up; the records down; the marked lines on the host             */
    double total_s;
} svt_vcf_update_info_times;
int svt_vcf_update_info_last_times(svt_vcf_update_info_times* times);
/* BND mates grouped in front of the paste (svtyper_amd/group_multiline.py; the reference's scripts/vcf_group_multiline.py).
 * Added without a new SVT_ABI_VERSION: probe for the symbol.  One call takes the WHOLE body (a pair may span the file).
 * format_table as svt_vcf_update_info_host's.  lines[j] is what the per-line rule (svt_vcf_group.h) reads of line j; plan is
 * the output in its order: entry {line, source} stands for `line`'s columns 1 to 5, FILTER and INFO with `source`'s QUAL,
 * FORMAT and sample columns (source == line for a line that is no BND; a pair is (a, a) then (b, a), a the line stored
 * first).  plan holds 2 * capacity entries.  Where the script dies, report->bad_line is that line's 1-based number, bad_kind
 * SVT_GROUP_BAD_*, bad_text the key or token in the way, and the plan ends in front of it (SVT_OK all the same).
 * svt_vcf_group_device: the same lines and the same plan, byte for byte, from svt_vcf_group_kernel.h; hash_bits (1..64):
 * the bits of the ID hashes it sorts by.  report->host_join: the join ran on the host (always for svt_vcf_group_host; for the
 * device where a line is marked or the file is not regular); n_bnd: the BND lines the join looked at (the host's
 * stops at the line the script dies on, the device's takes every line the rule decided).  svt_vcf_group_write: the text of the plan,
 * out_off[0 .. n_plan], kept for the calling thread (report->out_len, svt_vcf_group_take).                               */
typedef struct svt_group_line {
    uint64_t off;                           /* where the line begins in the text                                          */
    uint32_t len;                           /* its length without trailing blanks                                         */
    uint32_t id_b, id_n, mate_b, mate_n;    /* the ID column and INFO's MATEID value, relative to the line                */
    uint32_t flags;                         /* SVT_GROUP_BND, _HAS_MATE, _CI                                              */
    uint32_t slow;                          /* SVT_GROUP_SLOW_*: outside the rule's envelope, decided in plain C++        */
    uint32_t bad;                           /* SVT_GROUP_BAD_KEY | key << 8: the script dies ON this line (0: it does not) */
} svt_group_line;
typedef struct svt_group_out {
    uint32_t line, source;
} svt_group_out;
typedef struct svt_group_report {
    uint64_t out_len, host_lines, bad_line;
    uint32_t bad_kind, bad_sample;
    uint32_t host_join, n_bnd;
    char bad_text[48];
} svt_group_report;
#define SVT_GROUP_BND 1u                  /* SVTYPE=BND                                                                  */
#define SVT_GROUP_HAS_MATE 2u             /* a BND with a MATEID value                                                   */
#define SVT_GROUP_CI 4u                   /* what the script reads of the line's own intervals is there: CIPOS of a BND  */
                                          /* (read when it pairs), END, CIPOS and CIEND of any other line                */
#define SVT_GROUP_SLOW_HEAD 1u            /* fewer than eight columns, a POS or QUAL outside the exact rules             */
#define SVT_GROUP_SLOW_FORMAT 2u          /* FORMAT is not GT first and the header's keys in the header's order          */
#define SVT_GROUP_SLOW_BARE 4u            /* a key the script reads stands without '='                                   */
#define SVT_GROUP_SLOW_TOKEN 8u           /* END, or a token of CIPOS or CIEND, that is not '-'? and one to nine digits  */
#define SVT_GROUP_SLOW_ALT 16u            /* a BND with an empty ALT                                                     */
#define SVT_GROUP_SLOW 31u
#define SVT_GROUP_BAD_COLUMNS 1u          /* fewer than seven columns (IndexError)                                       */
#define SVT_GROUP_BAD_POS 2u              /* a POS that int() refuses (ValueError)                                       */
#define SVT_GROUP_BAD_QUAL 3u             /* a QUAL that float() refuses (ValueError)                                    */
#define SVT_GROUP_BAD_FORMAT 4u           /* a FORMAT key the header does not declare (the script's message, status 1)   */
#define SVT_GROUP_BAD_KEY 5u              /* bad_text: the INFO key the line lacks (KeyError)                            */
#define SVT_GROUP_BAD_NUMBER 6u           /* bad_text: a token of END, CIPOS or CIEND that int() refuses (ValueError)    */
#define SVT_GROUP_BAD_BARE 7u             /* bad_text: CIPOS or CIEND without '=' (AttributeError)                       */
#define SVT_GROUP_BAD_ALT 8u              /* a pair with an empty ALT (IndexError)                                       */
#define SVT_GROUP_BAD_EIGHT 9u            /* seven columns (the script's message, status 1)                              */
#define SVT_GROUP_KEY_SVTYPE 0u           /* the keys of SVT_GROUP_BAD_KEY in svt_group_line.bad                         */
#define SVT_GROUP_KEY_MATEID 1u
#define SVT_GROUP_KEY_END 2u
#define SVT_GROUP_KEY_CIPOS 3u
#define SVT_GROUP_KEY_CIEND 4u
int svt_vcf_group_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                       svt_group_line* lines, uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan,
                       svt_group_report* report);
int svt_vcf_group_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                         svt_group_line* lines, uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan,
                         svt_group_report* report, uint32_t hash_bits, int device);
int svt_vcf_group_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                        const uint8_t* format_table, uint64_t format_len, const svt_group_line* lines, uint64_t n_lines,
                        const svt_group_out* plan, uint64_t n_plan, uint64_t* out_off, svt_group_report* report);
int svt_vcf_group_take(uint8_t* out, uint64_t capacity);
/* the calling thread's most recent svt_vcf_group_device: its kernels by HIP events, its copies on the host's clock        */
typedef struct svt_vcf_group_times {
    double lines_kernels_s, scan_kernel_s, compact_kernels_s, sort_kernels_s, match_kernel_s, plan_kernels_s;
    double upload_s, download_s, host_s;    /* the text up; the records and the plan down; the host's join and report    */
    double total_s;
} svt_vcf_group_times;
int svt_vcf_group_last_times(svt_vcf_group_times* times);
/* The index fold: the uncompressed bytes of a .tbi (SAM spec 5.2 binning, 14-bit leaves, five levels; the layout of
 * the tabix format, format = 2 (VCF), col_seq 1, col_beg 2, col_end 0, meta '#', skip 0; pseudo-bin 37450 with the
 * contig's line count) for the body lines of `lines`, a table of the text as written.  The CHROM of line j is read at
 * text + (src_off ? src_off[j] : lines[j].off).  Payload k of the BGZF file holds text bytes [k * payload, ...) and
 * its member begins at file offset member_off[k]; member_off[n_members] is where the members end.  The result is kept
 * for the calling thread: *size is its length, svt_tbx_take copies it out.  A line the index cannot hold: *bad_line is
 * its 1-based number, *bad_kind why (SVT_OK, no result); 0 otherwise.                                                */
int svt_tbx_build(const uint8_t* text, uint64_t len, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n,
                  const uint64_t* member_off, uint64_t n_members, uint32_t payload, uint64_t* size, uint64_t* bad_line,
                  uint32_t* bad_kind);
int svt_tbx_take(uint8_t* out, uint64_t capacity);

/* ---- BAM records as spans: the coordinate-sorted, BAI-indexed `-w` dump (additions; the ABI number stays: probe for
 * svt_bam_spans_host) ----
 * svtyper_amd/csrc/svt_bam_sort_rules.h holds the per-record rule as one piece of source for the host and the device
 * (svt_bam_sort_kernel.h).  The records lie side by side in bytes[0, len), block_size first; record i is
 * bytes[rec_off[i] .. rec_off[i + 1]) -- rec_off holds n + 1 non-decreasing offsets, rec_off[n] <= len, and what lies in
 * front of rec_off[0] (the BAM header, for the writer) is nobody's record.  One span per record, in that order:
 *   off, len     where the record lies and how long it is (its block_size field included)
 *   key          tid' << 33 | (pos + 1) << 1 | reverse: tid' = tid, n_ref for tid = -1 (no coordinate: those go last);
 *                reverse is flag bit 0x10.  The order --sort-alignment writes is the stable order by key.
 *   tid, beg     refID and pos (0 for a record without coordinate)
 *   end          pos + the reference bases its CIGAR consumes (M, D, N, =, X); pos + 1 for an unmapped record (0x4), one
 *                without CIGAR or with a sum of 0; saturated at 2^32 - 1
 *   flags        SVT_BAM_UNMAPPED: flag 0x4.  SVT_BAM_NO_COOR: tid = -1.  SVT_BAM_BEYOND: end > 2^29, beyond what a BAI
 *                addresses (a CSI index holds it: svt_csi_build_bam).  SVT_BAM_BAD, with why: SVT_BAM_BAD_RECORD (the span is not
 *                36 bytes, block_size is not the span's length less 4, or the fixed part, name and CIGAR do not fit
 *                inside block_size), SVT_BAM_BAD_TID (tid >= n_ref or < -1), SVT_BAM_BAD_POS (pos < 0 with a tid,
 *                pos < -1 without); key, beg and end of such a span are 0.                                            */
typedef struct svt_bam_span {
    uint64_t off, len, key;
    int32_t tid;
    uint32_t beg, end, flags;
} svt_bam_span;
#define SVT_BAM_UNMAPPED 1u
#define SVT_BAM_NO_COOR 2u
#define SVT_BAM_BAD 4u
#define SVT_BAM_BEYOND 8u
#define SVT_BAM_BAD_RECORD 0x100u
#define SVT_BAM_BAD_TID 0x200u
#define SVT_BAM_BAD_POS 0x400u
/* what a record cannot be for svt_bam_sort_order / svt_bai_build (bad_kind) */
#define SVT_BAM_KIND_RECORD 1u   /* SVT_BAM_BAD_RECORD                                                                 */
#define SVT_BAM_KIND_TID 2u      /* SVT_BAM_BAD_TID                                                                    */
#define SVT_BAM_KIND_POS 3u      /* SVT_BAM_BAD_POS                                                                    */
#define SVT_BAM_KIND_BEYOND 4u   /* SVT_BAM_BEYOND (the index only)                                                    */
#define SVT_BAM_KIND_KEY_BACK 5u /* a key below the key of the record in front (the index only)                        */
/* The span table spans[0, n).  *key_and / *key_or (may be null): the AND and the OR of all keys (~0 and 0 for n = 0) --
 * a digit of the key in which they agree is one the sort can skip.                                                  */
int svt_bam_spans_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref,
                       svt_bam_span* spans, uint64_t* key_and, uint64_t* key_or);
int svt_bam_spans_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref,
                         svt_bam_span* spans, uint64_t* key_and, uint64_t* key_or, int device);
/* The stable order by key: perm[j] is the span that comes j-th (n entries, n < 2^32).  The host sorts with
 * std::stable_sort; the device with an LSD radix sort of (key, index) over the 8-bit digits in which the keys differ
 * (svt_radix_sort_kernel.h: a per-tile histogram, an exclusive scan and a stable scatter per digit; where an element goes is
 * a rank, so the permutation is a function of the keys alone).  A span with SVT_BAM_BAD: *bad_record is its 1-based number,
 * *bad_kind why (SVT_OK, perm undefined); 0 otherwise.                                                                 */
int svt_bam_sort_order_host(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind);
int svt_bam_sort_order_device(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind,
                              int device);
/* One call for the writer with deflate="device": bytes[0, len) -- the BAM header in front of rec_off[0], the records behind
 * it up to rec_off[n] = len -- goes up once; the span table and the keys are made there; with sort != 0 the keys are sorted
 * there and the records gathered behind the header into a second buffer; the stream as written is cut into members where
 * bam.BgzfWriter cuts it (the header in members of its own, whole records packed into at most 65 280 bytes, a longer
 * record cut at 65 280) and compressed by the kernels of svt_bgzf_deflate_device_mode (the same members, byte for byte).
 * out / capacity / out_off (member_capacity + 1 entries) as there; *n_members members were written, member k holds the
 * written stream's bytes [member_start[k], member_start[k + 1]) (member_capacity + 1 entries; n + len / 65280 + 2 members
 * always suffice).  spans[0, n): the table in WRITTEN order, off pointing into the written stream; perm[j]: which record
 * of the caller's was written j-th.  *bad_record / *bad_kind as svt_bam_sort_order (sort != 0: nothing is compressed).  */
int svt_bam_sorted_bgzf_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, int sort,
                               uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint64_t member_capacity,
                               uint64_t* n_members, uint64_t* member_start, svt_bam_span* spans, uint64_t* perm,
                               uint64_t* bad_record, uint32_t* bad_kind, int device);
/* the calling thread's most recent svt_bam_spans_device / _sort_order_device / _sorted_bgzf_device: its kernels by HIP
 * events, the three of the sort summed over its passes                                                               */
typedef struct svt_bam_sort_times {
    double keys_kernel_s, histogram_kernel_s, scan_kernel_s, scatter_kernel_s, gather_kernel_s;
    double total_s;             /* the whole call on the host's clock                                                */
    uint32_t passes;            /* digits the sort took                                                              */
    uint32_t reserved;
} svt_bam_sort_times;
int svt_bam_sort_last_times(svt_bam_sort_times* times);
/* ---- first occurrences of a record stream (additions; the ABI number stays: probe for svt_bam_first_host) ----
 * Which records of a stream (the layout of svt_bam_spans: bytes, len, rec_off with n + 1 non-decreasing offsets) are the first
 * with their key, in the caller's order.  The key is what `svtyper -w` writes a read once by: the l_read_name - 1 name bytes at
 * offset 36 and the 16-bit flag at offset 18 (svtyper_amd/csrc/svt_bam_first_rules.h: one piece of source for the host and the
 * device).  keep[i] = 1 iff no j < i has a key equal to record i's -- same flag, same length, same bytes --, else 0; *n_kept is
 * the sum of keep.  A record that is not well-formed (its span is below 36 bytes or leaves the bytes, block_size is not the
 * span's length less 4, l_read_name is 0, or 36 + l_read_name exceeds the span): *bad_record is the 1-based number of the first
 * such record (SVT_OK, keep undefined); 0 otherwise.  n = 0 is legal; n >= 2^32 or a decreasing rec_off is SVT_ERR_INVALID.
 * The host keeps a hash set of views into the bytes.  The device (svt_bam_first_kernel.h) hashes every record's key (FNV-1a,
 * 64 bits), sorts (hash, index) with the stable radix passes of svt_bam_sort_order_device, and lets one lane per sorted
 * position walk back over its run of equal hashes until it meets an equal key: the sort is stable, so what stands in front
 * of it there is earlier in the caller's order.  hash_bits (1..64, else SVT_ERR_INVALID; callers pass 64): how many low bits
 * of the hash are kept -- fewer make distinct keys share a run, which changes the cost and not the answer (tests).        */
int svt_bam_first_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept,
                       uint64_t* bad_record);
int svt_bam_first_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept,
                         uint64_t* bad_record, uint32_t hash_bits, int device);
/* the calling thread's most recent svt_bam_first_device: its kernels by HIP events, the three of the sort summed over its
 * passes                                                                                                              */
typedef struct svt_bam_first_times {
    double hash_kernel_s, histogram_kernel_s, scan_kernel_s, scatter_kernel_s, mark_kernel_s;
    double total_s;             /* the whole call on the host's clock                                                */
    uint32_t passes;            /* digits the sort took                                                              */
    uint32_t reserved;
} svt_bam_first_times;
int svt_bam_first_last_times(svt_bam_first_times* times);
/* The index fold: the bytes of a .bai ("BAI\1", n_ref; per reference its bins with their chunks -- a run of consecutive
 * records with one bin is one chunk --, pseudo-bin 37450 with (first start, last end) and (mapped, unmapped), and the
 * 16 kb linear index; n_bin = 0 and n_intv = 0 for a reference without records; the 64-bit n_no_coor at the end) for
 * `spans`, the table of a stream as written (spans[i].off rising, the records side by side).  Member k of the BGZF
 * file holds the stream's bytes [member_start[k], member_start[k + 1]) and begins at file offset member_off[k];
 * member_off[n_members] is where the members end.  A record with SVT_BAM_UNMAPPED and a tid is placed at its position
 * and counted as unmapped.  The result is kept for the calling thread: *size is its length, svt_bai_take copies it out.
 * A record the index cannot hold: *bad_record is its 1-based number, *bad_kind why (SVT_OK, no result); 0 otherwise.  */
int svt_bai_build(const svt_bam_span* spans, uint64_t n, int32_t n_ref, const uint64_t* member_start, const uint64_t* member_off,
                  uint64_t n_members, uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind);
int svt_bai_take(uint8_t* out, uint64_t capacity);

/* ---- a CSI index for the sorted `-w` BAM and the sorted VCF (additions; the ABI number stays: probe for svt_csi_build_bam) ----
 * The same fold as svt_bai_build / svt_tbx_build in a scheme (min_shift 14, depth): depth is the smallest d >= 5 for which
 * 2^(14 + 3 d) covers the file -- svt_csi_depth(max_end), with max_end the longest l_ref of a BAM header, or the largest end
 * among the body lines of a VCF's line table.  Positions are below 2^32, so depth is 5 or 6.  The bytes are the UNCOMPRESSED
 * CSIv1 (the writers put them through BGZF):
 *   header       "CSI\1", min_shift, depth, l_aux, aux, n_ref.  BAM: l_aux = 0.  VCF: aux is the tabix block -- seven 32-bit
 *                words format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, l_nm, then the NUL-terminated names --
 *                and n_ref the number of contigs
 *   per reference  n_bin; per bin, in rising order: bin, loffset, n_chunk, the chunks (a run of consecutive records with one
 *                bin is one chunk); then the pseudo-bin (8^(depth+1) - 1) / 7 + 1 with loffset 0 and the two chunks
 *                (first start, last end), (mapped, unmapped) -- (lines, 0) for a VCF; n_bin = 0 for a reference without records
 *   trailer      the 64-bit n_no_coor (0 for a VCF)
 *   loffset      of a bin: the virtual offset of the first record of that reference, in file order, that ends behind the
 *                bin's first position -- no record that overlaps a position at or behind the bin's start lies in front of it
 * Virtual offsets are svt_bai_build's: a position at a member's end is the next member's offset 0, the end of the data is
 * member_off[n_members] << 16.  A record or line whose end exceeds 2^(14 + 3 depth) or equals the saturated 0xFFFFFFFF is
 * refused as SVT_BAM_KIND_BEYOND / SVT_TBX_BEYOND: the decision comes from `end`, not from the SVT_BAM_BEYOND /
 * SVT_TBX_RANGE flag, which keeps meaning end > 2^29.  Arguments, result and refusals otherwise as svt_bai_build /
 * svt_tbx_build (KEY_BACK, CONTIG_AGAIN and POS_BACK included); svt_csi_take hands over the calling thread's last result
 * of either build or of the device fold.  Byte equality with htslib's .csi, or its choice of depth, is not claimed.      */
uint32_t svt_csi_depth(uint64_t max_end);
int svt_csi_build_bam(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                      const uint64_t* member_off, uint64_t n_members, uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind);
int svt_csi_build_vcf(const uint8_t* text, uint64_t len, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n,
                      const uint64_t* member_off, uint64_t n_members, uint32_t payload, uint64_t* size, uint64_t* bad_line,
                      uint32_t* bad_kind);
int svt_csi_take(uint8_t* out, uint64_t capacity);
/* The BAM's CSI fold on the device (svtyper_amd/csrc/svt_bam_index_kernel.h): svt_csi_build_bam's arguments and result, byte for
 * byte, over the caller's table -- one lane per record for virtual offset, bin and the first refusal (one 64-bit integer
 * minimum), one three-phase scan (per-tile partials, one workgroup over them, apply: no workgroup waits for another) carrying
 * the runs' numbers, the count of unmapped records and the running maximum of tid << 32 | end, the runs sorted by the radix
 * passes of svt_bam_sort_order_device, a bounded binary search per bin for its loffset and two per reference for its row.
 * What comes down is O(runs + n_ref): the sorted runs (key, start, end), the group heads' loffsets and a row per reference;
 * the host checks them (sorted, start <= end, heads consistent: SVT_ERR_HIP otherwise) and serialises them with the
 * serialiser of svt_csi_build_bam.  The bytes are left for svt_csi_take.                                               */
int svt_bam_index_fold_device(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                              const uint64_t* member_off, uint64_t n_members, uint64_t* size, uint64_t* bad_record,
                              uint32_t* bad_kind, int device);
/* svt_bam_sorted_bgzf_device with that fold behind the members: the stream goes up once and the spans are never uploaded
 * again -- after the members are made only member_start / out_off go up, n_members + 1 words each (out_off[k] is member k's
 * file offset: the members are the file).  *csi_size: the length of the .csi bytes left for svt_csi_take;
 * *index_bad_record / *index_bad_kind: the 1-based number, in WRITTEN order, of a record the index cannot hold and why (the
 * members are complete, no index bytes), 0 otherwise.  Everything else as svt_bam_sorted_bgzf_device; where that call
 * writes nothing (len = 0, or *bad_record != 0) there is no fold and *csi_size is 0.                                    */
int svt_bam_sorted_bgzf_csi_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref,
                                   uint64_t l_ref_max, int sort, uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off,
                                   uint64_t member_capacity, uint64_t* n_members, uint64_t* member_start, svt_bam_span* spans,
                                   uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, uint64_t* csi_size,
                                   uint64_t* index_bad_record, uint32_t* index_bad_kind, int device);
/* the calling thread's most recent device fold (either entry): its kernels by HIP events -- the scan's three phases summed,
 * the run-key kernel and the radix passes summed -- and the fold's time on the host's clock                            */
typedef struct svt_bam_index_times {
    double record_kernel_s, scan_kernel_s, sort_kernel_s, loffset_kernel_s, reference_kernel_s;
    double total_s;
    uint64_t runs;              /* runs of consecutive records with one bin                                             */
    uint32_t passes;            /* digits the runs' sort took                                                           */
    uint32_t reserved;
} svt_bam_index_times;
int svt_bam_index_last_times(svt_bam_index_times* times);

/* Verify: a property of the handle, off by default (0).  With it on, every call that takes the handle checks the
 * CRC-32 of every BGZF member it inflates, where it inflates it: the host reader's threads (libdeflate's or zlib's
 * crc32), or svt_crc32_kernel behind svt_inflate_kernel for the routes that inflate on the GPU (the expected values
 * go up with the member table).  A member that fails is treated as one that does not inflate: the host reader fails
 * the call with "BGZF block at offset N: CRC32 mismatch (stored 0x..., computed 0x...)", the walks flag its units
 * SVT_WALK_RANGE / answer SVT_LIBSCAN_MEMBER, and the host reader that then answers meets the same member.  With it
 * off nothing reads a trailer's CRC and nothing more is launched.  The blocks of the BAM header are read by
 * svt_bam_open, before the property can be set: they are not checked.                                           */
int svt_bam_set_verify(svt_bam* bam, int on);
int svt_bam_get_verify(const svt_bam* bam);

/* What verify did in the calling thread's most recent call that took a handle (thread-local, as svt_last_error's
 * text; zeros with verify off).  The members are counted on the handle: calls that use one handle from several
 * threads at the same time see each other's.                                                                    */
typedef struct svt_bgzf_verify_counts {
    uint64_t members_verified;  /* members whose CRC-32 was computed, on either side                             */
    uint64_t members_failed;    /* ... and differed                                                              */
    double host_crc_s;          /* in the host threads' CRC calls, summed over the threads                       */
    double device_crc_s;        /* svt_crc32_kernel, host-observed: launch to the statuses' arrival              */
} svt_bgzf_verify_counts;   /* (a C header cannot give a type and a function one name) */
int svt_bgzf_verify_stats(svt_bgzf_verify_counts* out);

/* svt_bam_evidence_walk_open_host: svt_bam_evidence_walk_host over the arena of the route below, with no GPU:
 * BAI lookup, a walk over BGZF headers only, every needed member inflated once by svt_inflate.h, one range per
 * index chunk from its start to its end virtual offset, and the walk ending each window where the fetch does
 * (the first record on another reference or at / behind the window's end).  A unit over a member that does
 * not inflate is flagged SVT_WALK_RANGE.                                                                    */
int svt_bam_evidence_walk_open_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                    svt_evidence* out, uint8_t* out_of_envelope, uint32_t* kept_reads);

/* svt_bam_evidence_device_inflate: svt_bam_evidence_device with the BGZF inflate on the GPU too.  The host does the
 * BAI lookup and the header walk and uploads the COMPRESSED members from the file mapping; svt_inflate_kernel
 * writes the arena in HBM; units over a member that failed go to the host reader (SVT_WALK_RANGE).  Arguments
 * and result are svt_bam_evidence_device's; `istats` (may be null) is filled; `count_host_blocks` != 0 also
 * builds the host-inflate arena of the same call, only to report how many blocks that route touches (the open
 * ranges of this one run to the end of every index chunk, the host reader stops at the first record behind the
 * window).  The arena is limited to 4 GiB of inflated bytes per call, as svt_bam_evidence_device's is.       */
typedef struct svt_evidence_inflate_stats {
    uint64_t blocks_inflated;      /* members handed to the inflate kernel                                   */
    uint64_t blocks_failed;        /* ... whose status is not 0                                              */
    uint64_t compressed_bytes;     /* uploaded                                                               */
    uint64_t inflated_bytes;       /* the arena                                                              */
    uint64_t blocks_host_route;    /* blocks the host-inflate arena holds (0 unless count_host_blocks)       */
    double host_index_s;           /* BAI lookup + header walk                                               */
    double compressed_upload_s;
    double inflate_kernel_s;       /* host-observed: launch to the statuses' arrival                         */
} svt_evidence_inflate_stats;

int svt_bam_evidence_device_inflate(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                    const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out,
                                    uint8_t* skipped, svt_evidence_device_stats* stats, svt_evidence_inflate_stats* istats,
                                    int count_host_blocks);

/* ---- the evidence dump of `svtyper -w` from the device reader (added under ABI 19 without a new number, like
 * svt_batch_verdicts: a library built before it lacks the symbols -- probe for svt_bam_evidence_device_dump) ----
 * The reads the reference writes to its -w BAM, as finished BAM records (block_size first; l_seq = 0, no sequence, no
 * qualities, XV:A:R|A set as classic.py:296-413 sets it), built where the alignment records already lie: the walk
 * (svt_evidence_walk.h) leaves one source row per evidence record, svtyper_amd/csrc/svt_dump_rules.h turns verdict bytes
 * (svt_batch_verdicts) + source rows + arena into the records, unit after unit, inside a unit fragment after fragment in
 * record order, inside a fragment its primary reads in arrival order.  The run-wide (query_name, flag) set stays the caller's.
 * Owned by the library: release with svt_evidence_dump_free.                                                          */
typedef struct svt_evidence_dump {
    uint8_t* bytes;               /* unit_offset[n_units] bytes                                                        */
    uint64_t* unit_offset;        /* n_units + 1: unit u's records are bytes[unit_offset[u] .. unit_offset[u + 1])     */
    uint8_t* unit_host;           /* n_units: 1 = this unit's reads must come from elsewhere (it was recomputed by the
                                     host reader, or it lies outside the dump's envelope); it has no bytes             */
    uint64_t n_bytes, n_reads;    /* bytes and records written                                                         */
    uint64_t units_dumped;        /* units with bytes                                                                  */
    uint64_t units_host;          /* units with unit_host = 1 ...                                                      */
    uint64_t units_outside_dump;  /* ... of them inside the walk's envelope and outside the dump's                     */
    double dump_s;                /* host-observed: the verdict kernel, both dump launches, the bytes' arrival         */
} svt_evidence_dump;
void svt_evidence_dump_free(svt_evidence_dump* d);

/* svt_bam_evidence_device_dump: svt_bam_evidence_device (inflate_on_device == 0; istats and count_host_blocks are ignored)
 * or svt_bam_evidence_device_inflate (!= 0) -- the same resident batch `*out` --, and behind it, on the call's stream,
 * svt_verdict_kernel over the new batch (its bytes stay in HBM) and the two launches of svt_dump_kernel.h.  The two
 * entries above launch and allocate nothing of this.                                                                  */
int svt_bam_evidence_device_dump(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                 const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out,
                                 uint8_t* skipped, svt_evidence_device_stats* stats, svt_evidence_inflate_stats* istats,
                                 int count_host_blocks, int inflate_on_device, svt_evidence_dump* dump);

/* The same with no GPU: svt_bam_evidence_walk_host with source rows, plus the dump rules on one lane.  There is no host
 * implementation of the verdicts: `verdicts` are handed IN, one byte per record in the record order of
 * svt_bam_evidence_walk_host on the same arguments (n_verdicts = its rec_offset[n_units]).  `out` / `out_of_envelope` are
 * svt_bam_evidence_walk_host's.  A unit outside the walk's or the dump's envelope has unit_host = 1 and no bytes.        */
int svt_bam_evidence_dump_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                    const uint8_t* verdicts, uint64_t n_verdicts, svt_evidence* out, uint8_t* out_of_envelope,
                                    svt_evidence_dump* dump);

/* Library statistics straight from the BAM (svtyper/parsers.py:501-576): what Library.from_bam scans
 * for, for ONE library given as its read-group ids, in three passes from the first record each --
 *   read_length : max query length (M/I/S/=/X) over the library's reads until 10 001 of them were seen
 *                 (calc_read_length, :516-528)
 *   hist        : Counter of template_length over the library's forward-strand, mate-reverse, mapped,
 *                 mate-mapped, primary reads with template_length > 0, until num_samp of them
 *                 (calc_insert_hist, :534-576; trimming and moments stay with the caller)
 *   in_lib/total: reads of the library among the first 100 000 records (calc_lib_prevalence, :501-513)
 * A read that has to be attributed but carries no RG tag is an error, as it is for the reference.   */
typedef struct svt_library_scan {
    int64_t read_length;
    uint64_t in_lib, total;
    uint64_t n_hist;          /* distinct template lengths                      */
    int64_t* hist_keys;       /* n_hist, in order of first occurrence (the order the
                                 reference's Counter sums in), malloc'ed        */
    uint64_t* hist_counts;    /* n_hist, malloc'ed                              */
} svt_library_scan;

int svt_bam_scan_library(const svt_bam* bam, uint32_t n_read_groups, const char* const* read_groups,
                         int64_t num_samp, svt_library_scan* out);
void svt_library_scan_free(svt_library_scan* s);

/* The scans of ALL libraries of a file in one walk over its record stream (svt_library_walk.h): the stream is cut
 * into segments at the record starts the BAI linear index knows, a segment is one wavefront's work
 * (svt_library_kernel.h) -- or one loop's on the host --, counted, capped against the three stop rules by a prefix
 * sum on the host, and accumulated into tables with integer atomics.  Library `l` is the read groups
 * read_groups[sum(rg_counts[0..l-1]) ...][rg_counts[l]]; out[l] is what svt_bam_scan_library gives for them, field
 * for field and key for key, and is released with svt_library_scan_free.  The stream is taken in rounds of at most
 * `round_bytes` of inflated bytes (0: the default, 64 MiB; 256 KiB .. 1 GiB otherwise), cut at segment starts.
 * Whatever lies outside the walk's envelope makes the whole call svt_bam_scan_library's, library by library:
 * stats->host_reason says why, and an error is the host scan's own (code and text).                      */
#define SVT_LIBSCAN_DEVICE 0        /* answered by the walk                                               */
#define SVT_LIBSCAN_NO_INDEX 1      /* the file has no index                                              */
#define SVT_LIBSCAN_TABLES 2        /* more libraries / read groups than the tables hold, a read group twice */
#define SVT_LIBSCAN_RECORD 3        /* a record beyond SVT_LIBSCAN_CAP_RECORD, malformed, or across a segment's end */
#define SVT_LIBSCAN_OVERFLOW 4      /* the overflow list is full                                          */
#define SVT_LIBSCAN_MEMBER 5        /* a BGZF member that is none or does not inflate                     */
#define SVT_LIBSCAN_NO_RG 6         /* a scanned record without a usable RG tag (also one behind every stop,
                                       when it lies in a round the walk took)                             */
#define SVT_LIBSCAN_INDEX 7         /* a linear-index offset that is not on the block chain               */
#define SVT_LIBSCAN_N_REASONS 8

typedef struct svt_library_scan_stats {
    uint64_t rounds, segments, members_inflated, compressed_bytes, inflated_bytes, overflow_entries, records_walked;
    double index_s, upload_s, inflate_s, count_s, accumulate_s, merge_s, host_scan_s;
    uint32_t host_reason;     /* SVT_LIBSCAN_*: 0, or why svt_bam_scan_library answered */
    uint32_t reserved;
} svt_library_scan_stats;

#define SVT_LIBSCAN_CAP_LIBRARIES 0
#define SVT_LIBSCAN_CAP_READ_GROUPS 1
#define SVT_LIBSCAN_CAP_DENSE_KEYS 2     /* K: template lengths below it have a slot per library        */
#define SVT_LIBSCAN_CAP_OVERFLOW 3       /* entries of the overflow list (template lengths >= K)         */
#define SVT_LIBSCAN_CAP_RECORD 4
#define SVT_LIBSCAN_CAP_ROUND_BYTES 5    /* the default round, in bytes                                  */
uint32_t svt_library_scan_capacity(int which);   /* SVT_LIBSCAN_CAP_*; 0 for an unknown one */
/* The overflow list of this thread's later calls holds `entries` (0, or more than the capacity: the capacity
 * again).  For tests of the full list.                                                                   */
void svt_library_scan_overflow_limit(uint32_t entries);

/* the whole route without a GPU: the same walk with one lane, members inflated by svt_inflate.h */
int svt_bam_scan_libraries_walk_host(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts,
                                     const char* const* read_groups, int64_t num_samp, uint64_t round_bytes,
                                     svt_library_scan* out, svt_library_scan_stats* stats);
/* on `device`.  inflate_on_device != 0: the host walks BGZF headers only, the compressed members are uploaded
 * from the file mapping and svt_inflate_kernel writes the arena; 0: host threads inflate, the arena is uploaded */
int svt_bam_scan_libraries_device(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts,
                                  const char* const* read_groups, int64_t num_samp, uint64_t round_bytes,
                                  int inflate_on_device, int device, svt_library_scan* out,
                                  svt_library_scan_stats* stats);

/* ---- CRAM 3.0 (additions without a new SVT_ABI_VERSION: probe for the symbols) ------------------------------------------
 * svtyper_amd/cram.py reads containers, blocks and indexes; what is native is the rANS 4x8 decoder (block method 4), once for
 * the host and the device (svt_rans.h), and the slice decoder (svt_cram.h).
 *
 * svt_rans_decode_*: block k is data[off[k], off[k + 1]) -- order byte, compressed size, uncompressed size, payload -- and decodes
 * to out[out_off[k], out_off[k] + out_size[k]).  status[k] is one of SVT_RANS_*; a block that is refused has its output range
 * zeroed.  Nothing outside the blocks' output ranges is changed.                                                            */
#define SVT_RANS_OK 0
#define SVT_RANS_HEADER 1       /* shorter than its header, an order other than 0 and 1, sizes that are not the block's      */
#define SVT_RANS_FREQ 2         /* the frequency table runs out, repeats itself or does not sum to 4096 (4095)               */
#define SVT_RANS_INPUT 3        /* the states or the renormalisation bytes run out                                           */
#define SVT_RANS_SYMBOL 4       /* a state points at no symbol of its context                                                */
#define SVT_RANS_SIZE 5         /* order 1 with nothing to decode                                                            */
int svt_rans_decode_host(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off,
                         const uint64_t* out_size, uint8_t* out, uint64_t out_len, uint32_t* status);
int svt_rans_decode_device(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off,
                           const uint64_t* out_size, uint8_t* out, uint64_t out_len, uint32_t* status, int device);
/* the calling thread's most recent svt_rans_decode_device: copies and kernels by HIP events, the call on the host's clock   */
typedef struct svt_rans_times {
    double upload_s, order0_kernel_s, order1_kernel_s, download_s;
    double total_s;
} svt_rans_times;
int svt_rans_last_times(svt_rans_times* times);

/* One slice as BAM records.  comp_header / slice_header: the content of the container's compression header block and of the
 * slice's header block; blocks / block_off / content_id / is_core: the slice's other blocks with their block method undone,
 * side by side; rg_ids: the SAM header's @RG ids in order, each ending in NUL; n_ref: the header's references.  The records --
 * block_size first, SEQ `N` x RL, QUAL 0xFF x RL -- are held for the calling thread: svt_cram_take copies info.bytes bytes and
 * info.n_records + 1 offsets.  A slice that is refused: SVT_ERR_INVALID, svt_last_error() says what was met.                  */
typedef struct svt_cram_slice_info {
    uint64_t n_records, bytes;
} svt_cram_slice_info;
int svt_cram_decode_slice(const uint8_t* comp_header, uint64_t comp_len, const uint8_t* slice_header, uint64_t slice_len,
                          const uint8_t* blocks, const uint64_t* block_off, const int32_t* content_id, const uint8_t* is_core,
                          uint32_t n_blocks, const char* rg_ids, uint32_t n_rg, int32_t n_ref, svt_cram_slice_info* info);
int svt_cram_take(uint8_t* records, uint64_t* rec_off);

#ifdef __cplusplus
}
#endif
#endif /* SVTYPER_READS_H */

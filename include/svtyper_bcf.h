/* svtyper_bcf.h -- VCF text as a BCF2.2 stream (VCFv4.3 specification, section 6): part of the C ABI of libsvtyper_hip.so.
 *
 * Additions; the ABI number stays: probe for svt_bcf_encode_host.  svtyper_amd/csrc/svt_bcf.h holds the record rule as one
 * piece of source for the host and the device (svt_bcf_kernel.h).
 *
 * `text[0, len)` is a whole VCF: the '#' lines up to and including the #CHROM line, then the data lines.  The header's
 * dictionaries are implicit (no IDX=): strings are PASS, then every ID of the ##FILTER, ##INFO and ##FORMAT lines in order of
 * first appearance, an ID of two categories once; contigs are the ##contig IDs in order.  The stream is the magic "BCF\2\2",
 * l_text, the header text as it stands in `text` and a NUL, then one record per data line, in text order or -- SVT_BCF_SORT --
 * in the stable (contig rank, POS) order of svt_vcf_sort_order.
 *
 * Nothing is repaired.  A line the header does not cover, or a token that is none of its declared type, stops the call: it
 * returns SVT_OK with info->bad_line (1-based, counted in `text`), bad_kind and bad_at (where in that line the key or token
 * begins) set, and nothing is held.  The lowest such line number is reported.
 */
#ifndef SVTYPER_BCF_H
#define SVTYPER_BCF_H

#include <stdint.h>

#include "svtyper_reads.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVT_BCF_KIND_COLUMNS 1u       /* fewer than 8 columns, or no data line at all                                   */
#define SVT_BCF_KIND_CONTIG 2u        /* CHROM is no ##contig of the header                                             */
#define SVT_BCF_KIND_POS 3u           /* POS is no number below 2^31 - 1                                                */
#define SVT_BCF_KIND_FILTER 4u        /* a FILTER name the header does not declare                                      */
#define SVT_BCF_KIND_INFO_KEY 5u      /* an INFO key the header does not declare                                        */
#define SVT_BCF_KIND_FORMAT_KEY 6u    /* a FORMAT key the header does not declare                                       */
#define SVT_BCF_KIND_INFO_VALUE 7u    /* an INFO token that is none of its key's Type (an integer outside int32's values too) */
#define SVT_BCF_KIND_FORMAT_VALUE 8u  /* the same in a sample, a GT allele that is no number, a sample with more fields than FORMAT */
#define SVT_BCF_KIND_SAMPLES 9u       /* a FORMAT column without samples, or a sample count that is not the header's    */
#define SVT_BCF_KIND_QUAL 10u         /* QUAL is no number                                                              */

#define SVT_BCF_SORT 1u               /* flags: the records in sorted order                                             */
#define SVT_BCF_EXACT_FLOATS 2u       /* flags (svt_bcf_encode_host): floats by the device's exact rule first, strtod for the
                                         rest -- info->host_lines then counts as the device route's does                  */

typedef struct svt_bcf_info {
    uint64_t bytes_len;         /* what svt_bcf_take hands over as `bytes`: the stream, or its BGZF members              */
    uint64_t n_offsets;         /* entries of `offsets` (records + 1, or members + 1)                                    */
    uint64_t n_records;
    uint64_t header_len;        /* bytes of the stream in front of the first record                                      */
    uint64_t stream_len;        /* bytes of the uncompressed stream                                                      */
    uint64_t bad_line;
    uint64_t host_lines;        /* lines with a float outside the device's envelope: encoded by the host twin            */
    uint64_t l_ref_max;         /* the longest declared contig                                                           */
    uint32_t bad_kind, bad_at;
    int32_t n_ref;              /* contigs of the header                                                                 */
    uint32_t n_sample;
} svt_bcf_info;

/* The stream of `text`, left for svt_bcf_take: bytes (header_len of header, then the records), offsets[0 .. n_records] (where
 * each record begins in the stream) and one span per record for the CSI fold (svt_csi_build_bam, svt_bam_index_fold_device:
 * off and len in the stream, tid, beg = POS - 1, end = beg + rlen, key = tid << 32 | beg, flags 0).  The device route makes the
 * line table and both passes over the lines on the GPU (one lane per line measures, the host sums the sizes, one lane per line
 * writes) and returns what the host route returns, byte for byte.                                                     */
int svt_bcf_encode_host(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info);
int svt_bcf_encode_device(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info, int device);
/* One call for the writer with deflate="device": the text goes up once, the stream is made there, cut every 65 280 bytes
 * and compressed by the deflate kernels (mode: SVT_DEFLATE_FIXED / SVT_DEFLATE_DYNAMIC).  Left for svt_bcf_take: bytes (the
 * members side by side, no EOF member), offsets[0 .. members] (where each begins in bytes), starts[0 .. members] (where each
 * member's payload begins in the stream) and the spans.                                                               */
int svt_bcf_bgzf_device(const uint8_t* text, uint64_t len, uint32_t flags, uint32_t mode, svt_bcf_info* info, int device);
/* hands over what the calling thread's last encoding call left, once: capacities in entries; starts may be null       */
int svt_bcf_take(uint8_t* bytes, uint64_t bytes_capacity, uint64_t* offsets, uint64_t offsets_capacity, uint64_t* starts,
                 svt_bam_span* spans, uint64_t spans_capacity);
/* the calling thread's most recent device call here: its two kernels by HIP events                                    */
typedef struct svt_bcf_times {
    double measure_kernel_s, write_kernel_s;
    double total_s;             /* the whole call on the host's clock                                                    */
} svt_bcf_times;
int svt_bcf_last_times(svt_bcf_times* times);

#ifdef __cplusplus
}
#endif
#endif /* SVTYPER_BCF_H */

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

/* ---- BCF2.2 records back to VCF text.  Additions; the ABI number stays: probe for svt_bcf_text_host.
 * svtyper_amd/csrc/svt_bcf_text.h holds the record rule as one piece of source for the host and the device
 * (svt_bcf_text_kernel.h: one wavefront per record, lanes over samples).
 *
 * `stream[0, len)` is a whole inflated BCF stream in host memory: the magic, l_text, the header text, the records.  The
 * dictionaries follow IDX= where a header line carries it and the implicit order of the writer above where none does.  The
 * text is the header without its ,IDX=n attributes and its NUL, then one line per record in the format of DESIGN 3.4: what
 * `bcftools view` is understood to print -- byte equality with htslib is not claimed, nothing here has htslib.
 *
 * Nothing is repaired.  A record the rule refuses stops the call: it returns SVT_OK with info->bad_record (1-based) and
 * bad_kind set, and nothing is held.  The lowest such record number is reported.  A stream that is no BCF (no magic, a header
 * without #CHROM line, two names at one IDX) is SVT_ERR_INVALID.                                                        */
#define SVT_BCF_TEXT_KIND_TRUNCATED 1u  /* the record runs out of the stream, or l_shared < 24                            */
#define SVT_BCF_TEXT_KIND_INDEX 2u      /* a contig, FILTER, INFO or FORMAT index the dictionaries do not hold            */
#define SVT_BCF_TEXT_KIND_SAMPLES 3u    /* n_sample is not the header's sample count                                      */
#define SVT_BCF_TEXT_KIND_TYPE 4u       /* a type code that is none of 0, 1, 2, 3, 5, 7, or one its field cannot have: ID and
                                           the alleles are characters, FILTER and every key integers, a key one integer   */
#define SVT_BCF_TEXT_KIND_COUNT 5u      /* a long count whose descriptor is not a single integer, or a vector beyond its part */
#define SVT_BCF_TEXT_KIND_GT 6u         /* a GT that is not held in an integer type                                       */
#define SVT_BCF_TEXT_KIND_LENGTH 7u     /* a shared or individual part whose walk does not end exactly at its length      */

#define SVT_BCF_TEXT_EXACT_FLOATS 2u    /* flags (svt_bcf_text_host): floats by the device's exact rule first, snprintf for
                                           the rest -- info->host_lines and the marks then count as the device route's do */

typedef struct svt_bcf_text_info {
    uint64_t text_len;          /* what svt_bcf_text_take hands over as `text`: header_len of header, then the lines      */
    uint64_t n_offsets;         /* entries of `offsets` (records + 1): where each record's line begins in the text        */
    uint64_t n_records;
    uint64_t header_len;
    uint64_t bad_record;
    uint64_t host_lines;        /* records with a float outside the device's envelope: written by the host twin           */
    uint64_t chunks;            /* pieces of at most block_bytes of stream, cut at record boundaries, the records ran in  */
    uint32_t bad_kind, n_sample;
} svt_bcf_text_info;

/* The text of `stream`, left for svt_bcf_text_take: text, offsets[0 .. n_records] and one mark per record (1: a float outside
 * the envelope -- on the host route only under SVT_BCF_TEXT_EXACT_FLOATS).  block_bytes: 0 for everything in one chunk.  The
 * device route uploads each chunk with its record offsets, measures (one text length and one mark per record), lets the host
 * take the exclusive sum, writes, downloads, and has the host twin write the marked records into their places: the host
 * route's text, byte for byte.                                                                                        */
int svt_bcf_text_host(const uint8_t* stream, uint64_t len, uint32_t flags, uint64_t block_bytes, svt_bcf_text_info* info);
int svt_bcf_text_device(const uint8_t* stream, uint64_t len, uint32_t flags, uint64_t block_bytes, svt_bcf_text_info* info, int device);
/* hands over what the calling thread's last decoding call left, once: capacities in entries                           */
int svt_bcf_text_take(uint8_t* text, uint64_t text_capacity, uint64_t* offsets, uint64_t offsets_capacity, uint8_t* marks,
                      uint64_t marks_capacity);
/* the calling thread's most recent device call here: kernels and copies by HIP events, summed over its chunks         */
typedef struct svt_bcf_text_times {
    double measure_kernel_s, write_kernel_s, upload_s, download_s;
    double total_s;             /* the whole call on the host's clock                                                    */
} svt_bcf_text_times;
int svt_bcf_text_last_times(svt_bcf_text_times* times);

#ifdef __cplusplus
}
#endif
#endif /* SVTYPER_BCF_H */

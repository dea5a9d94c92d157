// svt_library_walk.h -- alignment records in inflated BAM bytes -> what the three library scans of Library.from_bam compute
// (svt_bam_scan_library in svt_reads_library.h: read length, insert-size histogram, prevalence), for all libraries of a file at once.
//
// ONE piece of source for both places that run it, like svt_evidence_walk.h: the host (svt_bam_scan_libraries_walk_host, any
// C++17 compiler: where the walk is proven and sanitised) and the device (svt_library_kernel.h, hipcc, one wavefront per
// segment).  What a record means is svt_record_rules.h; a read group becomes a library through ew::find_name.
//
// The record stream is cut into SEGMENTS at record starts the BAI linear index knows (about every 16 kbp); the chain of
// block_size words, which only one lane can follow, is bounded per segment.  The three scans stop at a number of reads in file
// order (the 10 001st read of a library, its num_samp-th qualifying read, the 100 000th record), so a segment is walked twice:
//   count       per segment: its records, per library its reads and its qualifying reads (SegCount);
//   (host)      a prefix sum over the segments in file order turns the counts into caps per (segment, library) (SegCaps):
//               how many of the segment's records / reads / qualifying reads, in order, lie in front of each stop;
//   accumulate  the same walk; a read inside its caps goes into the tables with integer atomics only: count += 1, a 64-bit max
//               for the read length, a 64-bit min of (segment << 32 | record ordinal) for a key's first occurrence.  Integer
//               sums, minima and maxima do not depend on the order of arrival.
// Template lengths 1 .. kDenseKeys - 1 have a slot per library; a larger one is appended to the overflow list as
// (ordinal, key, library), which the host sorts and merges.
//
// The envelope.  Whatever the walk does not handle EXACTLY as the host scan does sets a reason (LW_*) for the segment; the
// caller then answers the whole call with svt_bam_scan_library.  No std::, no allocation, every access checked against the
// segment's end, every loop bounded by a length or a capacity.
#ifndef SVT_LIBRARY_WALK_H
#define SVT_LIBRARY_WALK_H

#include <stdint.h>

#include "svt_evidence_walk.h"
#include "svt_record_rules.h"

namespace svt {
namespace lw {

using namespace rr;

// ---- capacities -------------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxLibs = 16;               // libraries of one call
constexpr uint32_t kMaxReadGroups = 256;        // read groups of one call (a record's RG is looked up by a scan over them)
constexpr uint32_t kDenseKeys = 65536;          // K: template lengths 1 .. K - 1 have a slot per library (16 bytes each: 1 MiB per library)
constexpr uint32_t kOverflowCap = 1u << 20;     // entries of the overflow list (16 bytes each: 16 MiB)
constexpr uint32_t kMaxRecord = 1u << 16;       // bytes of one alignment record
constexpr uint32_t kBatch = 64;                 // chain records decoded side by side
constexpr uint64_t kReadLengthReads = 10001;    // calc_read_length looks at this many reads of a library
constexpr uint64_t kPrevalenceRecords = 100000; // calc_lib_prevalence looks at this many records of the file
constexpr uint32_t kNoCap = 0xFFFFFFFFu;
static_assert((uint64_t)kMaxLibs * kDenseKeys * 16 + (uint64_t)kOverflowCap * 16 <= (64ull << 20), "the tables stay far below the deep workspace's 256 MiB");

// ---- reasons (svt_library_scan_stats.host_reason: SVT_LIBSCAN_*) ------------------------------------------------------------
enum : uint32_t {
    LW_OK = 0,
    LW_NO_INDEX = 1,         // the file has no index
    LW_TABLES = 2,           // more libraries / read groups than the tables hold, or a read group named twice
    LW_RECORD = 3,           // a record larger than kMaxRecord, malformed, or not ending where its segment does
    LW_OVERFLOW = 4,         // the overflow list is full
    LW_MEMBER = 5,           // a BGZF member that is none or does not inflate
    LW_NO_RG = 6,            // a scanned record without a usable RG tag
    LW_INDEX = 7,            // a linear-index offset that is not on the block chain
    LW_N_REASONS = 8
};

// ---- what the caller hands over ---------------------------------------------------------------------------------------------
// arena offsets of the length word of the segment's first record and behind its last; `index` counts the call's segments in file
// order; `open` != 0: the arena ends inside the segment -- the walk stops in front of the first record that is not whole
struct Segment { uint32_t begin, end, index, open; };
struct SegCount {
    uint32_t n_records, status, unplaced, stop;      // `unplaced`: a record with refID < 0 ended it; `stop`: where the chain stopped
    uint32_t reads[kMaxLibs], qual[kMaxLibs];
};
struct SegCaps {
    uint32_t records, any;                           // `any` == 0: nothing of this segment lies in front of a stop
    uint32_t reads[kMaxLibs], qual[kMaxLibs];
};
struct Overflow { uint64_t ordinal; int32_t key; uint32_t lib; };
struct Tables {
    uint64_t* dense_count;                           // n_libs x kDenseKeys
    uint64_t* dense_first;                           // n_libs x kDenseKeys, ~0 while the key has not occurred
    uint64_t* read_length;                           // kMaxLibs
    uint64_t* in_lib;                                // kMaxLibs
    Overflow* overflow;                              // overflow_cap
    uint32_t* overflow_n;                            // entries asked for (more than overflow_cap: the list is full)
    uint32_t overflow_cap;
};
struct Params {
    const uint8_t* arena;
    uint64_t arena_len;
    const Segment* segments;
    const SegCaps* caps;                             // accumulate
    SegCount* counts;                                // count
    const ew::NameRef* rgs;                          // value: the read group's library
    const uint8_t* blob;
    uint32_t n_rgs, n_libs, n_segments;
    Tables T;
};

// the state of one segment's walk (LDS on the device)
struct Scratch {
    uint64_t qlen[kBatch];
    uint32_t off[kBatch], size[kBatch], ord[kBatch];
    int32_t tlen[kBatch];
    int8_t lib[kBatch];                              // -1: a read group of no library
    uint8_t kind[kBatch], qual[kBatch], acc[kBatch];
    uint32_t reads[kMaxLibs], nqual[kMaxLibs];
    uint32_t pos, nb, status, done, unplaced, n_records;
};
static_assert(sizeof(Scratch) == 1944, "the walk's LDS: svt_library_kernel.h and profiles/library_scan_kernel_resources.txt quote it");
enum : uint8_t { REC_OK = 0, REC_BAD = 1, REC_NO_RG = 2 };
enum : uint8_t { ACC_LENGTH = 1, ACC_HIST = 2, ACC_PREVALENCE = 4 };

// one lane, nothing shared: the atomics are plain arithmetic
struct HostCtx {
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
    static SVT_HD void add64(uint64_t* p, uint64_t v) { *p += v; }
    static SVT_HD void min64(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
    static SVT_HD void max64(uint64_t* p, uint64_t v) { if (v > *p) *p = v; }
    static SVT_HD uint32_t fetch_add32(uint32_t* p, uint32_t v) { const uint32_t was = *p; *p = was + v; return was; }
};

// ---- one record ---------------------------------------------------------------------------------------------------------------
SVT_HD bool qualifies(uint32_t flag, int32_t tlen)
{
    return !(flag & 0x10) && (flag & 0x20) && !(flag & (0x4 | 0x8)) && !(flag & (0x100 | 0x800)) && tlen > 0;
}
SVT_HD void eval_record(const Params& P, const uint8_t* d, uint32_t size, Scratch& S, uint32_t k)
{
    Core r;
    S.lib[k] = -1;
    S.qual[k] = 0;
    S.tlen[k] = 0;
    S.qlen[k] = 0;
    if (!decode_core(d, size, r)) { S.kind[k] = REC_BAD; return; }
    Tags t;
    tags_begin(t);
    uint32_t at = r.tags_off;
    if (walk_tags(d, size, at, /*stop_at_rg=*/true, t) != TAGS_AT_RG) { S.kind[k] = REC_NO_RG; return; }
    S.kind[k] = REC_OK;
    const int32_t rg = ew::find_name(P.rgs, P.n_rgs, P.blob, d + t.rg_off, t.rg_len);
    if (rg >= 0 && P.rgs[rg].value >= 0 && (uint32_t)P.rgs[rg].value < P.n_libs) S.lib[k] = (int8_t)P.rgs[rg].value;
    const int32_t tlen = (int32_t)ld32(d + 28);
    S.tlen[k] = tlen;
    S.qual[k] = qualifies(r.flag, tlen) ? 1 : 0;
    uint64_t n = 0;                                  // infer_query_length: M / I / S / = / X
    const uint8_t* cig = d + 32 + r.l_name;
    for (uint32_t c = 0; c < r.n_cigar; ++c) {
        const uint32_t w = ld32(cig + 4 * c);
        if (op_query(w & 0xF) || (w & 0xF) == 4) n += (uint64_t)(w >> 4);
    }
    S.qlen[k] = n;
}

// ---- one segment --------------------------------------------------------------------------------------------------------------
// kAccumulate == false: P.counts[si] is written.  true: the reads inside P.caps[si] go into P.T.
template <class X, bool kAccumulate>
SVT_HD void walk_segment(const Params& P, uint32_t si, Scratch& S)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const Segment sg = P.segments[si];
    if (kAccumulate && P.caps[si].any == 0) return;        // (the same for every lane)
    X::sync();
    if (lane == 0) {
        S.pos = sg.begin;
        S.nb = 0;
        S.status = (sg.end < sg.begin || (uint64_t)sg.end > P.arena_len) ? (uint32_t)LW_RECORD : (uint32_t)LW_OK;
        S.done = sg.begin >= sg.end ? 1u : 0u;
        S.unplaced = 0;
        S.n_records = 0;
        for (uint32_t l = 0; l < kMaxLibs; ++l) S.reads[l] = S.nqual[l] = 0;
    }
    X::sync();
    // (every pass takes at least one record or ends the segment: at most segment bytes / 36 / kBatch + 1 passes)
    while (S.status == LW_OK && !S.done) {
        X::sync();
        if (lane == 0) {                                   // the chain of block_size words
            uint32_t nb = 0, pos = S.pos;
            while (nb < kBatch && pos < sg.end) {
                if ((uint64_t)pos + 4 > sg.end) { if (sg.open) S.done = 1; else S.status = LW_RECORD; break; }
                const uint32_t size = ld32(P.arena + pos);
                if (size < 32 || size > kMaxRecord) { S.status = LW_RECORD; break; }
                if ((uint64_t)pos + 4 + size > sg.end) { if (sg.open) S.done = 1; else S.status = LW_RECORD; break; }
                if ((int32_t)ld32(P.arena + pos + 4) < 0) { S.unplaced = 1; S.done = 1; break; }   // the host scan stops here too
                S.off[nb] = pos + 4;
                S.size[nb] = size;
                ++nb;
                pos += 4 + size;
            }
            S.nb = nb;
            S.pos = pos;
            if (pos >= sg.end || nb == 0) S.done = 1;
        }
        X::sync();
        if (S.status != LW_OK) break;
        const uint32_t nb = S.nb;
        for (uint32_t k = lane; k < nb; k += lanes) eval_record(P, P.arena + S.off[k], S.size[k], S, k);
        X::sync();
        if (lane == 0) {                                   // the running counts, in file order
            uint32_t st = LW_OK;
            for (uint32_t k = 0; k < nb; ++k) {
                if (S.kind[k] == REC_BAD) { st = LW_RECORD; break; }
                if (S.kind[k] == REC_NO_RG) { st = LW_NO_RG; break; }
                const uint32_t ord = S.n_records++;
                uint8_t acc = 0;
                if (kAccumulate && ord < P.caps[si].records) acc |= ACC_PREVALENCE;
                const int32_t lib = S.lib[k];
                if (lib >= 0) {
                    const uint32_t nth = S.reads[lib]++;
                    if (kAccumulate && nth < P.caps[si].reads[lib]) acc |= ACC_LENGTH;
                    if (S.qual[k]) {
                        const uint32_t q = S.nqual[lib]++;
                        if (kAccumulate && q < P.caps[si].qual[lib]) acc |= ACC_HIST;
                    }
                }
                S.acc[k] = acc;
                S.ord[k] = ord;
            }
            if (st != LW_OK) S.status = st;
        }
        X::sync();
        if (S.status != LW_OK) break;
        if (kAccumulate) {
            for (uint32_t k = lane; k < nb; k += lanes) {
                const uint8_t acc = S.acc[k];
                const int32_t lib = S.lib[k];
                if (lib < 0 || !acc) continue;
                if (acc & ACC_LENGTH) X::max64(P.T.read_length + lib, S.qlen[k]);
                if (acc & ACC_PREVALENCE) X::add64(P.T.in_lib + lib, 1);
                if (acc & ACC_HIST) {
                    const uint64_t ordinal = ((uint64_t)sg.index << 32) | S.ord[k];
                    const uint32_t key = (uint32_t)S.tlen[k];          // (> 0: it qualifies)
                    if (key < kDenseKeys) {
                        const uint64_t slot = (uint64_t)lib * kDenseKeys + key;
                        X::add64(P.T.dense_count + slot, 1);
                        X::min64(P.T.dense_first + slot, ordinal);
                    } else {
                        const uint32_t at = X::fetch_add32(P.T.overflow_n, 1);
                        if (at < P.T.overflow_cap) P.T.overflow[at] = Overflow{ordinal, S.tlen[k], (uint32_t)lib};
                    }
                }
            }
        }
        X::sync();
    }
    X::sync();
    if (!kAccumulate && lane == 0) {
        SegCount& c = P.counts[si];
        c.n_records = S.n_records;
        c.status = S.status;
        c.unplaced = S.unplaced;
        c.stop = S.pos;
        for (uint32_t l = 0; l < kMaxLibs; ++l) { c.reads[l] = S.reads[l]; c.qual[l] = S.nqual[l]; }
    }
}

}  // namespace lw
}  // namespace svt

#endif  // SVT_LIBRARY_WALK_H

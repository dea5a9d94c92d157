// svt_evidence_walk.h -- alignment records in inflated BAM bytes -> the evidence records of one (breakpoint, sample) unit.
//
// ONE piece of source for both places that run it: the host (svt_bam_evidence_walk_host in svt_reads_walk.h, any C++17 compiler:
// this is where the walk is proven, fuzzed and sanitised) and the device (svt_evidence_kernel.h, hipcc, one workgroup per unit).
// What a record means -- its fixed fields, CIGAR, tags, aligned intervals, the split-read candidate -- is svt_record_rules.h,
// the same functions the host reader's process_unit calls.  The walk's own is here: its capacities and reasons, the two passes
// over a unit's record ranges, the fragment table behind a sort by name (a rank sort up to kMaxReads reads, sorted tiles and
// merges in the deep tier up to kMaxReadsDeep), the rows.  No std::, no allocation, every access checked against the length
// it was given, every loop bounded by a length or a capacity.
//
// The envelope.  Whatever the walk does not handle EXACTLY as the host reader does sets a reason (EW_*) for the unit and stops:
// the caller recomputes such a unit with process_unit (svt_bam_evidence_device) or returns it empty with its reason
// (svt_bam_evidence_walk_host).  The walk never guesses; it flags more readily than the host reader fails (a malformed tag the
// host would not have looked at still flags the unit), never less.
//
// Execution.  The per-unit functions are written once against a context `X`: X::lane() / X::lanes() / X::sync().  On the host
// there is one lane and sync() is nothing; on the device the lanes are the 256 threads of the unit's workgroup, the per-unit
// state (UnitScratch / DeepScratch) is LDS and the deep tier's tables are a slice of HBM.  Work is dealt out as
// `for (k = lane; k < n; k += lanes)`; what has to happen in arrival order (the chain of block_size words, the running counts
// of the max_reads rules, slot assignment) is lane 0's.
#ifndef SVT_EVIDENCE_WALK_H
#define SVT_EVIDENCE_WALK_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_geometry_math.h"
#include "svt_record_rules.h"

namespace svt {
namespace ew {

using namespace rr;

// ---- capacities (the LDS arithmetic is beside the kernels, svt_evidence_kernel.h) ---------------------------------------
// Kept reads come in two tiers of the same walk.  A unit of up to kMaxReads has its tables in UnitScratch (LDS on the device);
// one beyond that is flagged EW_READS by that tier WITH its true number of kept reads, and up to kMaxReadsDeep it is walked
// again with its tables in memory handed in (DeepScratch + Tables<uint32_t>: a slice of an HBM workspace on the device, the
// heap on the host).  Behind kMaxReadsDeep the unit stays EW_READS.
constexpr uint32_t kMaxReads = 1024;        // kept reads of one unit (both windows, after the flag / library filters): the LDS tier
constexpr uint32_t kMaxReadsDeep = 16384;   // ... the deep tier: what a unit is flagged EW_READS behind
constexpr uint32_t kSortTile = 2048;        // deep tier: (key, read) pairs sorted side by side in the staging area, then merged
constexpr uint32_t kMaxName = 128;          // query-name bytes of a kept read
constexpr uint32_t kMaxCigar = 256;         // CIGAR operations of a kept read, and of an SA entry
constexpr uint32_t kMaxSaEntries = 8;       // ';'-separated entries of an SA tag (more than one is discarded, as by the host)
constexpr uint32_t kMaxSaBytes = 1024;      // bytes of an SA value
constexpr uint32_t kMaxRecord = 1u << 16;   // bytes of one alignment record that is looked at
constexpr uint32_t kBatch = 256;            // chain records evaluated side by side

// ---- unit status ----------------------------------------------------------------------------------------------------------
enum : uint32_t {
    EW_OK = 0,
    EW_SKIPPED = 1,          // the max_reads rule of the host reader: the unit has no records (not a flag)
    EW_RANGE = 2,            // a record does not fit its arena range / bad block_size / record too long / bad window
    EW_READS = 3,            // more kept reads than the tier's capacity (S.n_reads is the true number all the same)
    EW_NAME = 4,             // query name longer than kMaxName
    EW_CIGAR = 5,            // more CIGAR operations than kMaxCigar
    EW_SA_CAP = 6,           // SA value beyond kMaxSaEntries / kMaxSaBytes
    EW_NO_RG = 7,            // no usable RG tag
    EW_UNKNOWN_RG = 8,       // RG not in the call's table / library index beyond the library table
    EW_MALFORMED = 9,        // malformed tag area, SA value or SA CIGAR
    EW_MAPQ = 10,            // SA MAPQ outside 0..255
    EW_N_STATUS = 11
};

// ---- what the caller hands over -----------------------------------------------------------------------------------------
struct Range { uint32_t begin, end; };     // arena offsets: the length word of the first record .. behind the last record
struct UnitRanges { uint32_t first; uint16_t n[2]; uint32_t preset; };   // ranges of window a, then of window b; preset != 0: status decided by the builder
struct NameRef { uint32_t off, len; int32_t value; };                     // bytes in `blob`: a read group (value = library index) or a reference name

struct Params {
    const uint8_t* arena;
    uint64_t arena_len;
    const Range* ranges;
    const UnitRanges* units;
    const svt_fetch_unit* windows;
    const svt_breakpoint* bps;
    const NameRef* rgs;
    const NameRef* refs;
    const uint8_t* blob;
    const double* lib_flank;
    uint32_t n_rgs, n_refs, n_libs;
    int32_t min_aligned, split_slop;
    int32_t count_mode;
    int64_t max_reads;
    uint32_t open_ranges;                  // != 0: a range ends at its chunk's end, not at the record that ends the fetch: the walk stops the window itself
};

// ---- the fixed-size summary of one kept read: what ReadInfo + SplitOut carry ---------------------------------------------
struct ReadSum {
    uint32_t name_off;                     // arena offset of the query name
    int32_t tid, start, end;               // (clip32'ed, as fill_read does)
    int32_t iv_s[2], iv_e[2];
    int32_t o_tid, o_start, o_end;         // the OTHER piece of the split candidate (the SA entry, or the dummy piece)
    uint16_t flag, lib;
    uint8_t name_len, mapq, o_mapq, bits;
};
enum : uint8_t { RS_NIV = 3, RS_REV = 4, RS_SPLIT = 8, RS_SOFT = 16, RS_SELF_LEFT = 32, RS_O_REV = 64, RS_DUP = 128 };

// ---- the source row of one record (the evidence dump of `svtyper -w`: svt_dump_rules.h) -----------------------------------
// Which alignment records a row was made of, and what the row's gated bytes cannot show.  rec[]: the arena offset of the
// block_size word of the row's primary ra, its primary rb, the read behind its seq candidate and the read behind its clip
// candidate; kNoRecord = absent.  bits: SRC_HIT_A / SRC_HIT_B = the UNGATED is_ref_seq_at answer, at breakend A or at B, for ra /
// rb (a hit with MAPQ 0 still tags the read R, classic.py:309-314; the record's gated MAPQ byte is 0 either way);
// SRC_CONTINUATION = the row continues the fragment of the row before.  Rows k = 0, 1, ... of a fragment list its primaries
// 2k and 2k + 1 in arrival order and the k-th seq / clip candidate: packer.FragmentSpan's ref_hits, seq[k] and clip[k].
struct SrcRow { uint32_t rec[4]; uint32_t bits; };
constexpr uint32_t kNoRecord = 0xffffffffu;
enum : uint32_t { SRC_HIT_A = 1, SRC_HIT_B = 2, SRC_CONTINUATION = 4 };
static_assert(sizeof(SrcRow) == 20, "a source row is five words");

// the staging area of kBatch chain records (`Idx`: what holds a slot of the tier's read table, all ones = none)
template <class Idx>
struct Batch {
    ReadSum rs[kBatch];
    uint32_t off[kBatch], size[kBatch], idx[kBatch], cnt[kBatch];
    Idx slot[kBatch];
    uint8_t ovl[kBatch], counted[kBatch], ev[kBatch], keep[kBatch];
};

// The tables of one unit, handed to the walk as pointers: `cap` summaries, keys, and three index arrays.  order[] carries the
// read's index with its top bit marking the first read of a run of one name; rows[] / rowoff[] hold rows per run and their
// running sum (at most one row per read, so whatever holds a read index holds them).
template <class IdxT>
struct Tables {
    typedef IdxT Idx;
    static constexpr IdxT kNoSlot = (IdxT) ~(IdxT)0;
    static constexpr IdxT kFirst = (IdxT)((IdxT)1 << (8 * sizeof(IdxT) - 1));
    static constexpr IdxT kIndex = (IdxT)(kFirst - 1);
    ReadSum* reads;
    uint64_t* key;
    IdxT *order, *rows, *rowoff;
    uint32_t cap;
};

// the LDS tier: everything of a unit in one block (72 240 bytes: two workgroups per CU)
struct UnitScratch {
    typedef uint16_t Idx;
    static constexpr bool kDeep = false;
    ReadSum reads[kMaxReads];
    union {
        Batch<uint16_t> b;                 // while the chain is walked
        struct {                           // afterwards
            uint64_t key[kMaxReads];
            uint16_t order[kMaxReads], rows[kMaxReads], rowoff[kMaxReads];
        } s;
    };
    uint32_t n_reads, n_walked, status, nb, pos, n_ovl, n_counted, lcp, n_rows, range_done, window_done;
    SVT_HD Tables<uint16_t> tables() { return Tables<uint16_t>{reads, s.key, s.order, s.rows, s.rowoff, kMaxReads}; }
};
static_assert(kMaxReads <= 0x7fff && kMaxReadsDeep <= 0x7fffffffu, "a read index and the first-of-run bit share an Idx");
static_assert(sizeof(Batch<uint16_t>) == 18944 && sizeof(UnitScratch) == 72240, "the LDS tier keeps its layout: two workgroups of the evidence kernel per CU (<= 80 KiB each)");

// the deep tier: the staging area and the sort's tile only (LDS on the device); the tables are the caller's (Tables<uint32_t>)
struct DeepScratch {
    typedef uint32_t Idx;
    static constexpr bool kDeep = true;
    union {
        Batch<uint32_t> b;                 // while the chain is walked
        struct {                           // while the reads are ordered
            uint64_t key[kSortTile];
            uint32_t idx[kSortTile];
        } t;
    };
    uint32_t n_reads, n_walked, status, nb, pos, n_ovl, n_counted, lcp, n_rows, range_done, window_done;
};
static_assert(sizeof(DeepScratch) <= 64 * 1024, "two workgroups of the deep kernel per CU");
// the tables of the deep tier as one slice of memory: summaries, keys, order / rows / rowoff
constexpr uint64_t kDeepSliceBytes = (uint64_t)kMaxReadsDeep * (sizeof(ReadSum) + sizeof(uint64_t) + 3 * sizeof(uint32_t));
static_assert(sizeof(ReadSum) == 52 && kDeepSliceBytes == 1179648, "1 179 648 bytes per slice");
SVT_HD Tables<uint32_t> deep_tables(uint8_t* slice)       // `slice`: kDeepSliceBytes, 8-byte aligned
{
    Tables<uint32_t> T;
    T.reads = reinterpret_cast<ReadSum*>(slice);
    T.key = reinterpret_cast<uint64_t*>(slice + (uint64_t)kMaxReadsDeep * sizeof(ReadSum));
    T.order = reinterpret_cast<uint32_t*>(T.key + kMaxReadsDeep);
    T.rows = T.order + kMaxReadsDeep;
    T.rowoff = T.rows + kMaxReadsDeep;
    T.cap = kMaxReadsDeep;
    return T;
}

struct HostCtx {
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
};

// ---- bytes ----------------------------------------------------------------------------------------------------------------
SVT_HD bool bytes_eq(const uint8_t* a, const uint8_t* b, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i) if (a[i] != b[i]) return false;
    return true;
}
// memcmp, then the shorter first: Python's order of ASCII names
SVT_HD int name_cmp(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb)
{
    const uint32_t n = na < nb ? na : nb;
    for (uint32_t i = 0; i < n; ++i) if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : na > nb ? 1 : 0;
}
// the LAST entry of the table with these bytes (a std::map / unordered_map filled in order keeps the last), or -1
SVT_HD int32_t find_name(const NameRef* tab, uint32_t n, const uint8_t* blob, const uint8_t* p, uint32_t len)
{
    for (uint32_t k = n; k-- > 0;)
        if (tab[k].len == len && bytes_eq(blob + tab[k].off, p, len)) return (int32_t)k;
    return -1;
}

// a run of 1..15 decimal digits (everything strtoll would read differently is outside the envelope)
SVT_HD bool digits(const uint8_t* p, uint32_t n, int64_t& v)
{
    if (n == 0 || n > 15) return false;
    v = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        v = v * 10 + (p[i] - '0');
    }
    return true;
}

// ---- one record -----------------------------------------------------------------------------------------------------------
// the split candidate of a primary read; EW_OK (candidate or not: RS_SPLIT in rs.bits) or a reason
SVT_HD uint32_t split_candidate(const Params& P, const uint8_t* d, const Core& r, const Tags& t, ReadSum& rs)
{
    if (r.n_cigar == 0) return EW_OK;
    CigarStats a;
    cigar_of_words(d + 32 + r.l_name, r.n_cigar, a);
    const bool a_rev = (r.flag & 0x10) != 0;
    if (!t.have_sa) {
        if (soft_clip_candidate(a, r.l_seq)) {
            rs.o_tid = -2; rs.o_start = 1; rs.o_end = 1; rs.o_mapq = 0;      // the dummy piece (chrom None)
            rs.bits |= (uint8_t)(RS_SPLIT | RS_SOFT | (a_rev ? RS_O_REV : 0) | (left_clipped(a) ? 0 : RS_SELF_LEFT));
        }
        return EW_OK;
    }
    if (t.sa_len > kMaxSaBytes) return EW_SA_CAP;
    const uint8_t* sa = d + t.sa_off;
    uint32_t fo[5], fl[5];
    uint32_t entries;
    const uint32_t fields = sa_fields(sa, t.sa_len, entries, fo, fl);
    if (entries > kMaxSaEntries) return EW_SA_CAP;
    if (entries > 1) return EW_OK;                                            // more than one entry: discarded
    if (fields < 5) return EW_MALFORMED;
    int64_t mate_pos1 = 0, mate_mapq = 0;
    if (!digits(sa + fo[1], fl[1], mate_pos1) || !digits(sa + fo[4], fl[4], mate_mapq)) return EW_MALFORMED;
    if (mate_mapq > 255) return EW_MAPQ;
    CigarStats b;
    const uint32_t cs = cigar_of_string(sa + fo[3], fl[3], kMaxCigar, 15, b);
    if (cs != CIGAR_OK) return cs == CIGAR_TOO_MANY ? EW_CIGAR : EW_MALFORMED;
    const int32_t b_at = find_name(P.refs, P.n_refs, P.blob, sa + fo[0], fl[0]);
    bool same_chrom = false;
    if (r.tid >= 0 && (uint32_t)r.tid < P.n_refs) {
        const NameRef& nr = P.refs[r.tid];
        same_chrom = nr.len == fl[0] && bytes_eq(P.blob + nr.off, sa + fo[0], fl[0]);
    }
    const bool b_rev = fl[2] == 1 && sa[fo[2]] == '-';
    const Piece pa = {r.tid, r.pos, r.end, a_rev, query_pos(a, a_rev)};
    const Piece pb = {b_at < 0 ? -3 : b_at, mate_pos1 - 1, mate_pos1 - 1 + b.ref, b_rev, query_pos(b, b_rev)};
    bool self_left;
    if (!split_valid(pa, pb, same_chrom, left_clipped(a), self_left)) return EW_OK;
    rs.o_tid = pb.tid; rs.o_start = clip32(pb.start); rs.o_end = clip32(pb.end); rs.o_mapq = (uint8_t)mate_mapq;
    rs.bits |= (uint8_t)(RS_SPLIT | (b_rev ? RS_O_REV : 0) | (self_left ? RS_SELF_LEFT : 0));
    return EW_OK;
}

// One record of the chain against one window.  `ovl`: pysam's overlap rule holds; `counted`: it counts for bam.count();
// `early` / `late`: reasons in front of / behind the count_mode 0 rule; `keep`: a read of the unit (rs is filled).
struct Eval { bool ovl, counted, keep; uint32_t early, late; };
SVT_HD void eval_record(const Params& P, const uint8_t* d, uint32_t size, uint32_t arena_off, int32_t wtid, int64_t lo, int64_t hi,
                        int64_t near_a, int64_t near_b, Eval& e, ReadSum& rs)
{
    e.ovl = e.counted = e.keep = false;
    e.early = e.late = EW_OK;
    Core r;
    if (!decode_core(d, size, r) || r.l_seq < 0 || r.tid != wtid || (int64_t)r.pos >= hi) { e.ovl = true; e.early = EW_RANGE; return; }   // (the builder ends a range in front of such a record)
    int64_t rend = r.end;
    if (r.n_cigar == 0 || rend <= r.pos) rend = (int64_t)r.pos + 1;
    if (!(rend > lo)) return;
    e.ovl = true;
    e.counted = !(r.flag & (0x4 | 0x100 | 0x200 | 0x400));
    if (r.flag & (0x4 | 0x400)) return;
    Tags t;
    tags_begin(t);
    uint32_t tags_at = r.tags_off;
    const bool tags_ok = walk_tags(d, size, tags_at, false, t) == TAGS_END;     // (a value that runs over the record's end counts as malformed here)
    if (!t.have_rg) { e.early = EW_NO_RG; return; }
    const int32_t at = find_name(P.rgs, P.n_rgs, P.blob, d + t.rg_off, t.rg_len);
    if (at < 0) { e.early = EW_UNKNOWN_RG; return; }
    const int32_t lib = P.rgs[at].value;
    if (lib < 0) return;                                   // library below the prevalence cut
    e.keep = true;
    if (!tags_ok) { e.late = EW_MALFORMED; return; }       // (a malformed tag behind RG)
    if ((uint32_t)lib >= P.n_libs || lib > 0xffff) { e.late = EW_UNKNOWN_RG; return; }
    const uint32_t name_len = r.l_name ? r.l_name - 1 : 0;
    if (name_len > kMaxName) { e.late = EW_NAME; return; }
    if (r.n_cigar > kMaxCigar) { e.late = EW_CIGAR; return; }
    rs.name_off = arena_off + 32;
    rs.name_len = (uint8_t)name_len;
    rs.tid = r.tid;
    rs.start = r.pos;
    rs.end = clip32(r.end);
    rs.iv_s[0] = rs.iv_s[1] = rs.iv_e[0] = rs.iv_e[1] = 0;
    rs.o_tid = rs.o_start = rs.o_end = 0;
    rs.flag = (uint16_t)r.flag;
    rs.lib = (uint16_t)lib;
    rs.mapq = (uint8_t)r.mapq;
    rs.o_mapq = 0;
    rs.bits = (uint8_t)((r.flag & 0x10) ? RS_REV : 0);
    if (r.flag & (0x100 | 0x800)) return;                  // secondary / supplementary: only its (name, flag) counts
    Intervals iv;
    aligned_intervals(d + 32 + r.l_name, r.n_cigar, r.pos, near_a, near_b, iv);
    rs.iv_s[0] = clip32(iv.s[0]); rs.iv_e[0] = clip32(iv.e[0]);
    rs.iv_s[1] = clip32(iv.s[1]); rs.iv_e[1] = clip32(iv.e[1]);
    rs.bits |= (uint8_t)iv.n;
    e.late = split_candidate(P, d, r, t, rs);
}

// ---- one unit ---------------------------------------------------------------------------------------------------------------
// the reads of one window's ranges into T.reads, in arrival order; stops with S.status set.  Behind T.cap reads the walk goes on
// and only counts (S.n_reads): walk_unit flags the unit once both windows are through.
template <class X, class SC>
SVT_HD void gather_window(const Params& P, SC& S, const Tables<typename SC::Idx>& T, const Range* ranges, uint32_t n_ranges, int32_t wtid, int64_t lo, int64_t hi,
                          int64_t near_a, int64_t near_b)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const bool mode1 = P.count_mode == 1 && P.max_reads >= 0, mode0 = P.count_mode == 0 && P.max_reads >= 0;
    typedef Tables<typename SC::Idx> Tb;
    if (lo < 0) lo = 0;                                    // (fetch clamps the window's start)
    X::sync();                                             // (every lane has read S.status on its way in)
    if (lane == 0) { S.n_ovl = 0; S.n_counted = 0; S.window_done = 0; }
    for (uint32_t ri = 0; ri < n_ranges; ++ri) {
        const Range rg = ranges[ri];
        X::sync();                                         // (every lane is past the status check that ended the range before)
        if (S.window_done) break;                          // (open ranges: the fetch ended in a range before this one)
        if (lane == 0) {
            S.pos = rg.begin;
            S.range_done = 0;
            if (rg.end < rg.begin || (uint64_t)rg.end > P.arena_len) { if (S.status == EW_OK) S.status = EW_RANGE; }
        }
        X::sync();
        // (every pass takes at least one record or ends the range: at most (range bytes / 36) / kBatch + 1 passes)
        while (S.status == EW_OK && !S.range_done) {
            X::sync();
            if (lane == 0) {                               // the chain of block_size words
                uint32_t nb = 0, pos = S.pos;
                while (nb < kBatch && pos < rg.end) {
                    if ((uint64_t)pos + 4 > rg.end) { S.status = EW_RANGE; break; }
                    const uint32_t size = ld32(P.arena + pos);
                    if (size < 32 || size > kMaxRecord || (uint64_t)pos + 4 + size > rg.end) { S.status = EW_RANGE; break; }
                    // the fetch's own stop rule (fetch() in svt_reads_records.h / build_arena in svt_reads_arena.h): the first record on another reference or at /
                    // behind the window's end ends the window
                    if (P.open_ranges && ((int32_t)ld32(P.arena + pos + 4) != wtid || (int64_t)(int32_t)ld32(P.arena + pos + 8) >= hi)) { S.window_done = 1; break; }
                    S.b.off[nb] = pos + 4;
                    S.b.size[nb] = size;
                    ++nb;
                    pos += 4 + size;
                }
                S.nb = nb;
                S.pos = pos;
                S.n_walked += nb;
                if (pos >= rg.end || nb == 0 || S.window_done) S.range_done = 1;
            }
            X::sync();
            if (S.status != EW_OK) break;
            const uint32_t nb = S.nb;
            for (uint32_t k = lane; k < nb; k += lanes) {
                Eval e;
                eval_record(P, P.arena + S.b.off[k], S.b.size[k], S.b.off[k], wtid, lo, hi, near_a, near_b, e, S.b.rs[k]);
                S.b.ovl[k] = e.ovl;
                S.b.counted[k] = e.counted;
                S.b.keep[k] = e.keep;
                S.b.ev[k] = (uint8_t)(e.early | (e.late << 4));
            }
            X::sync();
            if (lane == 0) {                               // the running counts and the slots, in arrival order
                uint32_t n_ovl = S.n_ovl, n_counted = S.n_counted, n_reads = S.n_reads, st = EW_OK;
                for (uint32_t k = 0; k < nb && st == EW_OK; ++k) {
                    S.b.slot[k] = Tb::kNoSlot;
                    if (!S.b.ovl[k]) continue;
                    const int64_t i = (int64_t)n_ovl++;    // enumerate() index of the fetch
                    const uint32_t early = S.b.ev[k] & 0xF, late = S.b.ev[k] >> 4;
                    if (early == EW_RANGE) { st = EW_RANGE; break; }
                    if (mode1 && S.b.counted[k] && (int64_t)++n_counted > P.max_reads) { st = EW_SKIPPED; break; }
                    if (early != EW_OK) { st = early; break; }
                    if (!S.b.keep[k]) continue;
                    if (mode0 && i > P.max_reads) { st = EW_SKIPPED; break; }
                    if (late != EW_OK) { st = late; break; }
                    if (n_reads < T.cap) S.b.slot[k] = (typename SC::Idx)n_reads;
                    ++n_reads;
                }
                S.n_ovl = n_ovl;
                S.n_counted = n_counted;
                S.n_reads = n_reads;
                if (st != EW_OK) S.status = st;
            }
            X::sync();
            if (S.status != EW_OK) break;
            for (uint32_t k = lane; k < nb; k += lanes)
                if (S.b.slot[k] != Tb::kNoSlot) T.reads[S.b.slot[k]] = S.b.rs[k];
            X::sync();
        }
        X::sync();
        if (S.status != EW_OK) return;
    }
}

SVT_HD ReadS absent_read() { ReadS r; r.tid = -1; r.start = r.end = r.iv0s = r.iv1s = r.iv0e = r.iv1e = 0; r.mapq = r.flags = r.extra = 0; return r; }
SVT_HD PieceS absent_piece() { PieceS p; p.tid = p.start = p.end = 0; p.mapq = p.flags = 0; return p; }
SVT_HD ReadS read_of_sum(const ReadSum& s)                 // fill_read + read_of
{
    ReadS r;
    r.tid = s.tid; r.start = s.start; r.end = s.end;
    r.iv0s = s.iv_s[0]; r.iv1s = s.iv_s[1]; r.iv0e = s.iv_e[0]; r.iv1e = s.iv_e[1];
    r.mapq = s.mapq;
    r.flags = SVT_READ_PRESENT | ((s.bits & RS_REV) ? SVT_READ_REVERSE : 0);
    r.extra = 0;
    return r;
}
SVT_HD PieceS piece_of_sum(const ReadSum& s, bool left)    // fill_piece + piece_of: the read itself or the other piece
{
    PieceS p;
    const bool self = ((s.bits & RS_SELF_LEFT) != 0) == left;
    if (self) { p.tid = s.tid; p.start = s.start; p.end = s.end; p.mapq = s.mapq; p.flags = SVT_READ_PRESENT | ((s.bits & RS_REV) ? SVT_READ_REVERSE : 0); }
    else { p.tid = s.o_tid; p.start = s.o_start; p.end = s.o_end; p.mapq = s.o_mapq; p.flags = SVT_READ_PRESENT | ((s.bits & RS_O_REV) ? SVT_READ_REVERSE : 0); }
    return p;
}

SVT_HD bool is_primary(const ReadSum& s) { return !(s.bits & RS_DUP) && !(s.flag & (0x100 | 0x800)); }
SVT_HD bool same_name(const Params& P, const ReadSum& a, const ReadSum& b)
{
    return a.name_len == b.name_len && bytes_eq(P.arena + a.name_off, P.arena + b.name_off, a.name_len);
}

// ---- the order of a unit's reads: T.order[rank] = read, by (query name, arrival) -- a total order, so every correct sort
// gives the same permutation.  T.key holds the eight name bytes behind the common prefix; whole names are compared only
// between equal keys.
template <class Idx>
SVT_HD bool read_before(const Params& P, const Tables<Idx>& T, uint64_t ka, uint32_t a, uint64_t kb, uint32_t b)
{
    if (ka != kb) return ka < kb;
    const int c = name_cmp(P.arena + T.reads[a].name_off, T.reads[a].name_len, P.arena + T.reads[b].name_off, T.reads[b].name_len);
    return c != 0 ? c < 0 : a < b;
}

// the LDS tier: rank = reads in front of this one, n * n key compares side by side
template <class X, class Idx>
SVT_HD void order_by_rank(const Params& P, const Tables<Idx>& T, uint32_t n)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    for (uint32_t k = lane; k < n; k += lanes) {
        const uint64_t key = T.key[k];
        const ReadSum& me = T.reads[k];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint64_t kj = T.key[j];
            bool less;
            if (kj != key) less = kj < key;
            else if (j == k) less = false;
            else {
                const int c = name_cmp(P.arena + T.reads[j].name_off, T.reads[j].name_len, P.arena + me.name_off, me.name_len);
                less = c != 0 ? c < 0 : j < k;
            }
            rank += less ? 1u : 0u;
        }
        T.rowoff[k] = (Idx)rank;
    }
    X::sync();
    for (uint32_t k = lane; k < n; k += lanes) T.order[T.rowoff[k]] = (Idx)k;
    X::sync();
}

// The deep tier: O(n log^2 n).  Tiles of kSortTile (key, read) pairs are sorted in the staging area (a bitonic network: pairs
// (i, i + stride) side by side, neighbouring lanes on neighbouring pairs -- at stride 1 the 8-byte keys of a wave lie 16 bytes
// apart, a two-way bank conflict, every other stride reads consecutive keys); the sorted tiles are merged pairwise through
// T.order and T.rows (free until the rows are counted), every element finding its place in the other run by a binary search
// over T.key[] of that run's reads: log2(n / kSortTile) <= 3 passes, each reads its source in order and gathers ~log2(run)
// keys per element from a table of n * 12 bytes that stays in L2.
constexpr uint32_t kSortPad = 0xffffffffu;                     // fills a tile behind its last pair: sorts behind every read
template <class X>
SVT_HD void order_deep(const Params& P, DeepScratch& S, const Tables<uint32_t>& T, uint32_t n)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    auto before = [&](uint64_t ka, uint32_t a, uint64_t kb, uint32_t b) {
        if (a == kSortPad || b == kSortPad) return a != kSortPad;      // (pad against pad: never swapped, either way)
        return read_before(P, T, ka, a, kb, b);
    };
    for (uint32_t t0 = 0; t0 < n; t0 += kSortTile) {              // (at most kMaxReadsDeep / kSortTile tiles)
        const uint32_t m = n - t0 < kSortTile ? n - t0 : kSortTile;
        uint32_t tile = 2;
        while (tile < m) tile <<= 1;                               // (<= kSortTile)
        X::sync();
        for (uint32_t k = lane; k < tile; k += lanes) {
            S.t.key[k] = k < m ? T.key[t0 + k] : ~0ull;
            S.t.idx[k] = k < m ? t0 + k : kSortPad;
        }
        X::sync();
        for (uint32_t size = 2; size <= tile; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                for (uint32_t k = lane; k < tile / 2; k += lanes) {
                    const uint32_t i = 2 * k - (k & (stride - 1)), j = i + stride;
                    const uint64_t ki = S.t.key[i], kj = S.t.key[j];
                    const uint32_t ri = S.t.idx[i], rj = S.t.idx[j];
                    const bool up = (i & size) == 0;
                    if (up ? before(kj, rj, ki, ri) : before(ki, ri, kj, rj)) {
                        S.t.key[i] = kj; S.t.idx[i] = rj;
                        S.t.key[j] = ki; S.t.idx[j] = ri;
                    }
                }
                X::sync();
            }
        }
        for (uint32_t k = lane; k < m; k += lanes) T.order[t0 + k] = S.t.idx[k];
    }
    X::sync();
    uint32_t* src = T.order;
    uint32_t* dst = T.rows;
    for (uint32_t run = kSortTile; run < n; run <<= 1) {          // (at most log2(kMaxReadsDeep / kSortTile) passes)
        for (uint32_t k = lane; k < n; k += lanes) {
            const uint32_t base = k / (2 * run) * (2 * run);
            const uint32_t mid = base + run < n ? base + run : n, end = base + 2 * run < n ? base + 2 * run : n;
            const bool left = k < mid;
            const uint32_t me = src[k];
            const uint64_t key = T.key[me];
            uint32_t lo = left ? mid : base, hi = left ? end : mid;   // the other run: how many of it come in front of me
            const uint32_t first = lo;
            for (uint32_t it = 0; it < 32 && lo < hi; ++it) {
                const uint32_t at = lo + (hi - lo) / 2, other = src[at];
                if (read_before(P, T, T.key[other], other, key, me)) lo = at + 1;
                else hi = at;
            }
            dst[base + (k - (left ? base : mid)) + (lo - first)] = me;
        }
        X::sync();
        uint32_t* const was = src;
        src = dst;
        dst = was;
    }
    if (src != T.order) {
        for (uint32_t k = lane; k < n; k += lanes) T.order[k] = src[k];
        X::sync();
    }
}

// The whole unit.  `out` == nullptr: count only.  Results: S.status, S.n_rows, S.n_reads, S.n_walked (valid on every lane
// after the call).  `out` holds S.n_rows records in sorted(query_name) order, as process_unit emits them.  `S`: UnitScratch or
// DeepScratch; `T`: the tier's tables (UnitScratch::tables() / deep_tables()).  S.n_reads is the unit's number of kept reads
// also when that is more than T.cap: the unit is EW_READS then.
// kSrc (the evidence dump): the write pass also leaves one SrcRow per record in `src`; without it -- every instantiation there
// was before the dump -- or with `src` null the walk is what it is without.
template <class X, class SC, bool kSrc = false>
SVT_HD void walk_unit(const Params& P, uint64_t u, SC& S, const Tables<typename SC::Idx>& T, Record4* out, SrcRow* src = nullptr)
{
    typedef typename SC::Idx Idx;
    typedef Tables<Idx> Tb;
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const UnitRanges ur = P.units[u];
    const svt_fetch_unit w = P.windows[u];
    const svt_breakpoint bp = P.bps[u];
    if (lane == 0) { S.n_reads = 0; S.n_walked = 0; S.n_rows = 0; S.status = ur.preset; S.lcp = 0; }
    X::sync();
    if (S.status == EW_OK) gather_window<X>(P, S, T, P.ranges + ur.first, ur.n[0], w.tid_a, w.lo_a, w.hi_a, bp.pos_a, bp.pos_b);
    X::sync();
    if (S.status == EW_OK) gather_window<X>(P, S, T, P.ranges + ur.first + ur.n[0], ur.n[1], w.tid_b, w.lo_b, w.hi_b, bp.pos_a, bp.pos_b);
    X::sync();
    if (lane == 0 && S.status == EW_OK && S.n_reads > T.cap) S.status = EW_READS;
    X::sync();
    if (S.status != EW_OK) return;
    const uint32_t n = S.n_reads;
    if (n == 0) return;

    // ---- order by (query name, arrival): the common prefix once, then eight bytes behind it as the key
    {
        uint32_t lcp = T.reads[0].name_len;
        const uint8_t* a = P.arena + T.reads[0].name_off;
        for (uint32_t k = lane; k < n; k += lanes) {
            const uint8_t* b = P.arena + T.reads[k].name_off;
            const uint32_t m = lcp < T.reads[k].name_len ? lcp : T.reads[k].name_len;
            uint32_t i = 0;
            while (i < m && a[i] == b[i]) ++i;
            lcp = i;
        }
        T.rows[lane] = (Idx)lcp;                      // (lanes() <= kMaxReads: a slot per lane)
        X::sync();
        if (lane == 0) {
            uint32_t m = T.rows[0];
            for (uint32_t k = 1; k < lanes; ++k) m = T.rows[k] < m ? T.rows[k] : m;
            S.lcp = m;
        }
        X::sync();
    }
    const uint32_t lcp = S.lcp;
    for (uint32_t k = lane; k < n; k += lanes) {
        const uint8_t* p = P.arena + T.reads[k].name_off + lcp;
        const uint32_t have = T.reads[k].name_len - lcp;
        uint64_t key = 0;
        for (uint32_t i = 0; i < 8; ++i) key = (key << 8) | (i < have ? p[i] : 0u);
        T.key[k] = key;
    }
    X::sync();
    if constexpr (SC::kDeep) order_deep<X>(P, S, T, n);
    else order_by_rank<X>(P, T, n);
    // ---- fragments: runs of one name; the top bit of order[] marks the first read of a run
    for (uint32_t p = lane; p < n; p += lanes) {
        const bool first = p == 0 || !same_name(P, T.reads[T.order[p] & Tb::kIndex], T.reads[T.order[p - 1] & Tb::kIndex]);
        T.rows[p] = first ? 1 : 0;
    }
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes)
        if (T.rows[p]) T.order[p] |= Tb::kFirst;
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes) {              // the same (name, flag) again: dropped
        ReadSum& me = T.reads[T.order[p] & Tb::kIndex];
        bool dup = false;
        for (uint32_t q = p; q > 0 && !(T.order[q] & Tb::kFirst) && !dup;) {
            --q;
            dup = T.reads[T.order[q] & Tb::kIndex].flag == me.flag;
        }
        if (dup) me.bits |= RS_DUP;
    }
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes) {              // rows of the fragment: max(1, ceil(primaries / 2), |seq|, |clip|)
        uint32_t rows = 0;
        if (T.order[p] & Tb::kFirst) {
            uint32_t np = 0, ns = 0, nc = 0;
            for (uint32_t q = p; q < n && (q == p || !(T.order[q] & Tb::kFirst)); ++q) {
                const ReadSum& m = T.reads[T.order[q] & Tb::kIndex];
                if (!is_primary(m)) continue;
                ++np;
                if (m.bits & RS_SPLIT) { if (m.bits & RS_SOFT) ++nc; else ++ns; }
            }
            rows = (np + 1) / 2;
            rows = rows < 1 ? 1 : rows;
            rows = rows < ns ? ns : rows;
            rows = rows < nc ? nc : rows;
        }
        T.rows[p] = (Idx)rows;
    }
    X::sync();
    if (lane == 0) {
        uint32_t at = 0;
        for (uint32_t p = 0; p < n; ++p) { T.rowoff[p] = (Idx)at; at += T.rows[p]; }
        S.n_rows = at;
    }
    X::sync();
    if (!out) return;
    for (uint32_t p = lane; p < n; p += lanes) {
        const uint32_t rows = T.rows[p];
        if (!rows) continue;
        uint32_t end = p + 1;
        while (end < n && !(T.order[end] & Tb::kFirst)) ++end;
        const uint32_t lib = T.reads[T.order[p] & Tb::kIndex].lib;        // SamFragment(read, lib): the first read's
        uint32_t np = 0;
        for (uint32_t q = p; q < end; ++q) np += is_primary(T.reads[T.order[q] & Tb::kIndex]) ? 1u : 0u;
        uint32_t qp = p, qs = p, qc = p;                   // cursors: next primary / seq candidate / clip candidate
        for (uint32_t k = 0; k < rows; ++k) {
            ReadS ra = absent_read(), rb = absent_read();
            PieceS sl = absent_piece(), sr = absent_piece(), cl = absent_piece(), cr = absent_piece();
            SrcRow row = {{kNoRecord, kNoRecord, kNoRecord, kNoRecord}, k > 0 ? (uint32_t)SRC_CONTINUATION : 0u};   // (dead without kSrc)
            for (int j = 0; j < 2; ++j) {
                while (qp < end && !is_primary(T.reads[T.order[qp] & Tb::kIndex])) ++qp;
                if (qp < end) {
                    const ReadSum& m = T.reads[T.order[qp] & Tb::kIndex];
                    (j ? rb : ra) = read_of_sum(m);
                    if constexpr (kSrc) row.rec[j] = m.name_off - 36;      // (the name lies 32 bytes into the record, behind block_size)
                    ++qp;
                }
            }
            for (; qs < end; ++qs) {
                const ReadSum& m = T.reads[T.order[qs] & Tb::kIndex];
                if (is_primary(m) && (m.bits & RS_SPLIT) && !(m.bits & RS_SOFT)) {
                    sl = piece_of_sum(m, true); sr = piece_of_sum(m, false);
                    if constexpr (kSrc) row.rec[2] = m.name_off - 36;
                    ++qs;
                    break;
                }
            }
            for (; qc < end; ++qc) {
                const ReadSum& m = T.reads[T.order[qc] & Tb::kIndex];
                if (is_primary(m) && (m.bits & RS_SPLIT) && (m.bits & RS_SOFT)) {
                    cl = piece_of_sum(m, true); cr = piece_of_sum(m, false);
                    if constexpr (kSrc) row.rec[3] = m.name_off - 36;
                    ++qc;
                    break;
                }
            }
            ra.extra = lib;
            rb.extra = ((k == 0 && np == 2) ? SVT_FRAG_PAIR : 0u) | (k > 0 ? SVT_FRAG_CONTINUATION : 0u);
            out[T.rowoff[p] + k] = geometry_record(ra, rb, sl, sr, cl, cr, bp, P.lib_flank[lib], P.min_aligned, P.split_slop);
            if constexpr (kSrc) {
                if (src) {
                    const int32_t m = P.min_aligned;
                    if (is_ref_seq_at(ra, bp.tid_a, bp.pos_a, m) || is_ref_seq_at(ra, bp.tid_b, bp.pos_b, m)) row.bits |= SRC_HIT_A;
                    if (is_ref_seq_at(rb, bp.tid_a, bp.pos_a, m) || is_ref_seq_at(rb, bp.tid_b, bp.pos_b, m)) row.bits |= SRC_HIT_B;
                    src[T.rowoff[p] + k] = row;
                }
            }
        }
    }
    X::sync();
}

}  // namespace ew
}  // namespace svt

#endif  // SVT_EVIDENCE_WALK_H

// svt_evidence_walk.h -- alignment records in inflated BAM bytes -> the evidence records of one (breakpoint, sample) unit.
//
// ONE piece of source for both places that run it: the host (svt_bam_evidence_walk_host in svt_reads.cpp, any C++17 compiler:
// this is where the walk is proven, fuzzed and sanitised) and the device (svt_evidence_kernel.h, hipcc, one workgroup per unit).
// It restates what decode_core / decode_rest / find_z_tag / aligned_intervals / split_candidate / parse_cigar_string and
// process_unit of svt_reads.cpp compute, as plain functions over `const uint8_t*` + length: no std::, no allocation, every
// access checked against the length it was given, every loop bounded by a length or a capacity.
//
// The envelope.  Whatever the walk does not handle EXACTLY as the host reader does sets a reason (EW_*) for the unit and stops:
// the caller recomputes such a unit with process_unit (svt_bam_evidence_device) or returns it empty with its reason
// (svt_bam_evidence_walk_host).  The walk never guesses; it flags more readily than the host reader fails (a malformed tag the
// host would not have looked at still flags the unit), never less.
//
// Execution.  The per-unit functions are written once against a context `X`: X::lane() / X::lanes() / X::sync().  On the host
// there is one lane and sync() is nothing; on the device the lanes are the 256 threads of the unit's workgroup and the
// per-unit state (UnitScratch) is LDS.  Work is dealt out as `for (k = lane; k < n; k += lanes)`; what has to happen in
// arrival order (the chain of block_size words, the running counts of the max_reads rules, slot assignment) is lane 0's.
#ifndef SVT_EVIDENCE_WALK_H
#define SVT_EVIDENCE_WALK_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_geometry_math.h"

namespace svt {
namespace ew {

// ---- capacities (the LDS arithmetic is beside the kernel, svt_evidence_kernel.h) ----------------------------------------
constexpr uint32_t kMaxReads = 1024;        // kept reads of one unit (both windows, after the flag / library filters)
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
    EW_READS = 3,            // more kept reads than kMaxReads
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

struct UnitScratch {
    ReadSum reads[kMaxReads];
    union {
        struct {                           // while the chain is walked
            ReadSum rs[kBatch];
            uint32_t off[kBatch], size[kBatch], idx[kBatch], cnt[kBatch];
            uint16_t slot[kBatch];
            uint8_t ovl[kBatch], counted[kBatch], ev[kBatch], keep[kBatch];
        } b;
        struct {                           // afterwards
            uint64_t key[kMaxReads];
            uint16_t order[kMaxReads], rows[kMaxReads], rowoff[kMaxReads];
        } s;
    };
    uint32_t n_reads, n_walked, status, nb, pos, n_ovl, n_counted, lcp, n_rows, range_done;
};

struct HostCtx {
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
};

// ---- bytes ----------------------------------------------------------------------------------------------------------------
SVT_HD uint32_t ld32(const uint8_t* d) { return (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24); }
SVT_HD int32_t clip32(int64_t x) { return (int32_t)(x < (int64_t)INT32_MIN ? (int64_t)INT32_MIN : x > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : x); }
SVT_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
SVT_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
SVT_HD int64_t abs64(int64_t a) { return a < 0 ? -a : a; }
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

// ---- CIGAR ------------------------------------------------------------------------------------------------------------------
SVT_HD bool op_clip(uint32_t op) { return op == 4 || op == 5; }
SVT_HD bool op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
SVT_HD bool op_query(uint32_t op) { return op == 0 || op == 1 || op == 7 || op == 8; }
SVT_HD bool op_aligned(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// what query_pos_from_cigar / left_clipped / the clip rules need of a CIGAR, gathered in one forward pass
struct CigarStats {
    uint32_t n, first_op, last_op;
    int64_t first_len, last_len, query, clips, ref;
};
SVT_HD void cigar_begin(CigarStats& c) { c.n = 0; c.first_op = c.last_op = 0; c.first_len = c.last_len = c.query = c.clips = c.ref = 0; }
SVT_HD void cigar_add(CigarStats& c, uint32_t op, int64_t len)
{
    if (c.n == 0) { c.first_op = op; c.first_len = len; }
    c.last_op = op; c.last_len = len;
    ++c.n;
    if (op_clip(op)) c.clips += len;
    else if (op_query(op)) c.query += len;
    if (op_ref(op)) c.ref += len;
}
struct QPos { int64_t start, end, length; };
// query_pos_from_cigar: the clip the walk meets first (the last operation of a reverse read) opens the query
SVT_HD QPos query_pos(const CigarStats& c, bool reverse)
{
    QPos q;
    int64_t lead = 0;
    if (c.n) {
        const uint32_t op = reverse ? c.last_op : c.first_op;
        if (op_clip(op)) lead = reverse ? c.last_len : c.first_len;
    }
    q.start = lead;
    q.end = lead + c.query;
    q.length = c.clips + c.query;
    return q;
}
SVT_HD bool left_clipped(const CigarStats& c)
{
    const bool lc = op_clip(c.first_op), rc = op_clip(c.last_op);
    return (lc && !rc) || (lc && rc && c.first_len > c.last_len);
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

// parse_cigar_string; EW_OK, EW_MALFORMED or EW_CIGAR
SVT_HD uint32_t cigar_of_string(const uint8_t* s, uint32_t n, CigarStats& c)
{
    cigar_begin(c);
    int64_t num = 0;
    uint32_t nd = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t ch = s[i];
        if (ch >= '0' && ch <= '9') {
            if (++nd > 15) return EW_MALFORMED;
            num = num * 10 + (ch - '0');
            continue;
        }
        uint32_t op;
        switch (ch) {
        case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'N': op = 3; break; case 'S': op = 4; break;
        case 'H': op = 5; break; case 'P': op = 6; break; case '=': op = 7; break; case 'X': op = 8; break;
        default: return EW_MALFORMED;
        }
        if (nd == 0) return EW_MALFORMED;
        if (c.n >= kMaxCigar) return EW_CIGAR;
        cigar_add(c, op, num);
        num = 0;
        nd = 0;
    }
    return nd ? EW_MALFORMED : EW_OK;
}

// ---- one record -----------------------------------------------------------------------------------------------------------
struct Core {
    int32_t tid, pos, l_seq;
    uint32_t l_name, n_cigar, flag, mapq, tags_off;
    int64_t end;
};
// decode_core: false when the variable-length parts do not fit `size`
SVT_HD bool decode_core(const uint8_t* d, uint32_t size, Core& r)
{
    if (size < 32) return false;
    r.tid = (int32_t)ld32(d);
    r.pos = (int32_t)ld32(d + 4);
    r.l_name = d[8];
    r.mapq = d[9];
    r.n_cigar = (uint32_t)d[12] | ((uint32_t)d[13] << 8);
    r.flag = (uint32_t)d[14] | ((uint32_t)d[15] << 8);
    r.l_seq = (int32_t)ld32(d + 16);
    uint64_t off = 32;
    if (off + r.l_name + 4ull * r.n_cigar > size) return false;
    off += r.l_name;
    r.end = r.pos;
    for (uint32_t k = 0; k < r.n_cigar; ++k) {
        const uint32_t c = ld32(d + off + 4 * k);
        if (op_ref(c & 0xF)) r.end += (int64_t)(c >> 4);
    }
    off += 4ull * r.n_cigar;
    if (r.l_seq < 0) return false;         // (the host reader's size_t arithmetic rejects it the same way)
    off += (uint64_t)(((int64_t)r.l_seq + 1) / 2 + (int64_t)r.l_seq);
    if (off > size) return false;
    r.tags_off = (uint32_t)off;
    return true;
}

// the whole tag area, validated; the first RG:Z and the first SA:Z values (offset into the record, length without the NUL)
struct Tags { uint32_t rg_off, rg_len, sa_off, sa_len; bool have_rg, have_sa; };
SVT_HD bool walk_tags(const uint8_t* d, uint32_t size, uint32_t from, Tags& t)
{
    t.have_rg = t.have_sa = false;
    t.rg_off = t.rg_len = t.sa_off = t.sa_len = 0;
    uint64_t i = from;
    const uint64_t n = size;
    while (i + 3 <= n) {
        const uint8_t a0 = d[i], a1 = d[i + 1], ty = d[i + 2];
        i += 3;
        uint64_t skip = 0;
        switch (ty) {
        case 'A': case 'c': case 'C': skip = 1; break;
        case 's': case 'S': skip = 2; break;
        case 'i': case 'I': case 'f': skip = 4; break;
        case 'Z': case 'H': {
            uint64_t q = i;
            while (q < n && d[q]) ++q;
            if (q >= n) return false;
            if (ty == 'Z' && a0 == 'R' && a1 == 'G' && !t.have_rg) { t.have_rg = true; t.rg_off = (uint32_t)i; t.rg_len = (uint32_t)(q - i); }
            if (ty == 'Z' && a0 == 'S' && a1 == 'A' && !t.have_sa) { t.have_sa = true; t.sa_off = (uint32_t)i; t.sa_len = (uint32_t)(q - i); }
            skip = q - i + 1;
            break;
        }
        case 'B': {
            if (i + 5 > n) return false;
            const uint8_t sub = d[i];
            const uint32_t cnt = ld32(d + i + 1);
            const uint64_t sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            skip = 5 + (uint64_t)cnt * sz;
            break;
        }
        default: return false;
        }
        i += skip;
        if (i > n) return false;                            // a value that runs over the end of the record
    }
    return true;
}

// aligned_intervals: all gap-free aligned intervals when there are at most two, else the two nearest to the breakends in the
// order of a stable sort by distance
SVT_HD void aligned_intervals(const uint8_t* cig, uint32_t n_cigar, int64_t pos, int64_t near_a, int64_t near_b, ReadSum& out)
{
    int64_t fs[2] = {0, 0}, fe[2] = {0, 0};        // the first two, in order
    int64_t bs[2] = {0, 0}, be[2] = {0, 0}, bd[2] = {0, 0};   // the two nearest, nearest first
    uint32_t n = 0;
    int64_t p = pos, cs = 0, ce = 0;
    bool open = false;
    auto close = [&]() {
        auto one = [&](int64_t q) { return (cs <= q && q <= ce) ? (int64_t)0 : min64(abs64(cs - q), abs64(ce - q)); };
        const int64_t dist = min64(one(near_a), one(near_b));
        if (n < 2) { fs[n] = cs; fe[n] = ce; }
        if (n == 0) { bs[0] = cs; be[0] = ce; bd[0] = dist; }
        else if (n == 1) {
            if (dist < bd[0]) { bs[1] = bs[0]; be[1] = be[0]; bd[1] = bd[0]; bs[0] = cs; be[0] = ce; bd[0] = dist; }
            else { bs[1] = cs; be[1] = ce; bd[1] = dist; }
        } else if (dist < bd[0]) { bs[1] = bs[0]; be[1] = be[0]; bd[1] = bd[0]; bs[0] = cs; be[0] = ce; bd[0] = dist; }
        else if (dist < bd[1]) { bs[1] = cs; be[1] = ce; bd[1] = dist; }
        ++n;
    };
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t c = ld32(cig + 4 * k), op = c & 0xF;
        const int64_t len = (int64_t)(c >> 4);
        if (op_aligned(op)) {
            if (!open) { cs = p; open = true; }
            ce = p + len;
            p += len;
        } else if (op == 2 || op == 3) {
            if (open) close();
            open = false;
            p += len;
        }
    }
    if (open) close();
    const uint32_t keep = n < 2 ? n : 2;
    for (uint32_t k = 0; k < 2; ++k) {
        const bool have = k < keep;
        out.iv_s[k] = have ? clip32(n > 2 ? bs[k] : fs[k]) : 0;
        out.iv_e[k] = have ? clip32(n > 2 ? be[k] : fe[k]) : 0;
    }
    out.bits = (uint8_t)((out.bits & ~RS_NIV) | keep);
}

// split_candidate for a primary read; EW_OK (candidate or not: RS_SPLIT in rs.bits) or a reason
SVT_HD uint32_t split_candidate(const Params& P, const uint8_t* d, const Core& r, const Tags& t, ReadSum& rs)
{
    if (r.n_cigar == 0) return EW_OK;
    const uint8_t* cig = d + 32 + r.l_name;
    CigarStats a;
    cigar_begin(a);
    for (uint32_t k = 0; k < r.n_cigar; ++k) {
        const uint32_t c = ld32(cig + 4 * k);
        cigar_add(a, c & 0xF, (int64_t)(c >> 4));
    }
    const bool a_rev = (r.flag & 0x10) != 0;
    if (!t.have_sa) {
        const bool fc = op_clip(a.first_op), lc = op_clip(a.last_op);
        if (!(fc || lc)) return EW_OK;
        const int64_t clip_length = max64(fc ? a.first_len : 0, lc ? a.last_len : 0);
        if (clip_length > 0 && ((int64_t)r.l_seq - a.query) <= 50) {
            rs.o_tid = -2; rs.o_start = 1; rs.o_end = 1; rs.o_mapq = 0;      // the dummy piece (chrom None)
            rs.bits |= (uint8_t)(RS_SPLIT | RS_SOFT | (a_rev ? RS_O_REV : 0) | (left_clipped(a) ? 0 : RS_SELF_LEFT));
        }
        return EW_OK;
    }
    // SA:Z:chrom,pos,strand,CIGAR,mapQ,NM;...
    if (t.sa_len > kMaxSaBytes) return EW_SA_CAP;
    const uint8_t* sa = d + t.sa_off;
    uint32_t len = t.sa_len;
    while (len && sa[len - 1] == ';') --len;
    uint32_t entries = 1;
    for (uint32_t i = 0; i < len; ++i) if (sa[i] == ';') ++entries;
    if (entries > kMaxSaEntries) return EW_SA_CAP;
    if (entries > 1) return EW_OK;                                            // more than one entry: discarded
    uint32_t fo[5] = {0, 0, 0, 0, 0}, fl[5] = {0, 0, 0, 0, 0}, n_fld = 0, p0 = 0;
    for (uint32_t i = 0; i <= len; ++i) {
        if (i == len || sa[i] == ',') {
            if (n_fld < 5) { fo[n_fld] = p0; fl[n_fld] = i - p0; }
            ++n_fld;
            p0 = i + 1;
        }
    }
    if (n_fld < 5) return EW_MALFORMED;
    int64_t mate_pos1 = 0, mate_mapq = 0;
    if (!digits(sa + fo[1], fl[1], mate_pos1) || !digits(sa + fo[4], fl[4], mate_mapq)) return EW_MALFORMED;
    if (mate_mapq > 255) return EW_MAPQ;
    CigarStats b;
    const uint32_t cs = cigar_of_string(sa + fo[3], fl[3], b);
    if (cs != EW_OK) return cs;
    const int32_t b_at = find_name(P.refs, P.n_refs, P.blob, sa + fo[0], fl[0]);
    const int32_t b_tid = b_at < 0 ? -3 : b_at;
    const int64_t b_start = mate_pos1 - 1, b_end = b_start + b.ref;
    const bool b_rev = fl[2] == 1 && sa[fo[2]] == '-';
    bool same_chrom = false;
    if (r.tid >= 0 && (uint32_t)r.tid < P.n_refs) {
        const NameRef& nr = P.refs[r.tid];
        same_chrom = nr.len == fl[0] && bytes_eq(P.blob + nr.off, sa + fo[0], fl[0]);
    }
    const bool self_left = same_chrom ? !((int64_t)r.pos > b_start) : !left_clipped(a);
    const QPos qa = query_pos(a, a_rev), qb = query_pos(b, b_rev);
    const QPos &l = self_left ? qa : qb, &rq = self_left ? qb : qa;
    const int64_t shared = max64(0, 1 + min64(l.end, rq.end) - max64(l.start, rq.start));
    const int64_t non_overlap = min64(1 + l.end - l.start - shared, 1 + rq.end - rq.start - shared);
    if (non_overlap < 20) return EW_OK;
    const int32_t l_tid = self_left ? r.tid : b_tid, r_tid = self_left ? b_tid : r.tid;
    const bool l_rev = self_left ? a_rev : b_rev, r_rev = self_left ? b_rev : a_rev;
    if (l_tid == r_tid && l_rev == r_rev) {
        const int64_t l_start = self_left ? (int64_t)r.pos : b_start, l_end = self_left ? r.end : b_end;
        const int64_t r_start = self_left ? b_start : (int64_t)r.pos, r_end = self_left ? b_end : r.end;
        const int64_t l_sd = l_start - (l_rev ? l.length - l.end : l.start), l_ed = l_end - (l_rev ? l.length - l.start : l.end);
        const int64_t r_sd = r_start - (r_rev ? rq.length - rq.end : rq.start), r_ed = r_end - (r_rev ? rq.length - rq.start : rq.end);
        const int64_t ins = l_rev ? r_ed - l_sd : l_ed - r_sd;
        if (abs64(ins) < 50) return EW_OK;
        const int64_t desert = rq.start - l.end - 1;
        if (desert > 0 && desert - max64(0, ins) > 50) return EW_OK;
    }
    rs.o_tid = b_tid; rs.o_start = clip32(b_start); rs.o_end = clip32(b_end); rs.o_mapq = (uint8_t)mate_mapq;
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
    if (!decode_core(d, size, r) || r.tid != wtid || (int64_t)r.pos >= hi) { e.ovl = true; e.early = EW_RANGE; return; }   // (the builder ends a range in front of such a record)
    int64_t rend = r.end;
    if (r.n_cigar == 0 || rend <= r.pos) rend = (int64_t)r.pos + 1;
    if (!(rend > lo)) return;
    e.ovl = true;
    e.counted = !(r.flag & (0x4 | 0x100 | 0x200 | 0x400));
    if (r.flag & (0x4 | 0x400)) return;
    Tags t;
    const bool tags_ok = walk_tags(d, size, r.tags_off, t);
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
    aligned_intervals(d + 32 + r.l_name, r.n_cigar, r.pos, near_a, near_b, rs);
    e.late = split_candidate(P, d, r, t, rs);
}

// ---- one unit ---------------------------------------------------------------------------------------------------------------
template <class X>
SVT_HD void set_status(UnitScratch& S, uint32_t st)
{
    if (X::lane() == 0 && S.status == EW_OK) S.status = st;
}

// the reads of one window's ranges into S.reads, in arrival order; stops with S.status set
template <class X>
SVT_HD void gather_window(const Params& P, UnitScratch& S, const Range* ranges, uint32_t n_ranges, int32_t wtid, int64_t lo, int64_t hi,
                          int64_t near_a, int64_t near_b)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const bool mode1 = P.count_mode == 1 && P.max_reads >= 0, mode0 = P.count_mode == 0 && P.max_reads >= 0;
    if (lo < 0) lo = 0;                                    // (fetch clamps the window's start)
    X::sync();                                             // (every lane has read S.status on its way in)
    if (lane == 0) { S.n_ovl = 0; S.n_counted = 0; }
    for (uint32_t ri = 0; ri < n_ranges; ++ri) {
        const Range rg = ranges[ri];
        X::sync();                                         // (every lane is past the status check that ended the range before)
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
                    S.b.off[nb] = pos + 4;
                    S.b.size[nb] = size;
                    ++nb;
                    pos += 4 + size;
                }
                S.nb = nb;
                S.pos = pos;
                S.n_walked += nb;
                if (pos >= rg.end || nb == 0) S.range_done = 1;
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
                    S.b.slot[k] = 0xffff;
                    if (!S.b.ovl[k]) continue;
                    const int64_t i = (int64_t)n_ovl++;    // enumerate() index of the fetch
                    const uint32_t early = S.b.ev[k] & 0xF, late = S.b.ev[k] >> 4;
                    if (early == EW_RANGE) { st = EW_RANGE; break; }
                    if (mode1 && S.b.counted[k] && (int64_t)++n_counted > P.max_reads) { st = EW_SKIPPED; break; }
                    if (early != EW_OK) { st = early; break; }
                    if (!S.b.keep[k]) continue;
                    if (mode0 && i > P.max_reads) { st = EW_SKIPPED; break; }
                    if (late != EW_OK) { st = late; break; }
                    if (n_reads >= kMaxReads) { st = EW_READS; break; }
                    S.b.slot[k] = (uint16_t)n_reads++;
                }
                S.n_ovl = n_ovl;
                S.n_counted = n_counted;
                S.n_reads = n_reads;
                if (st != EW_OK) S.status = st;
            }
            X::sync();
            if (S.status != EW_OK) break;
            for (uint32_t k = lane; k < nb; k += lanes)
                if (S.b.slot[k] != 0xffff) S.reads[S.b.slot[k]] = S.b.rs[k];
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

// The whole unit.  `out` == nullptr: count only.  Results: S.status, S.n_rows, S.n_reads, S.n_walked (valid on every lane
// after the call).  `out` holds S.n_rows records in sorted(query_name) order, as process_unit emits them.
template <class X>
SVT_HD void walk_unit(const Params& P, uint64_t u, UnitScratch& S, Record4* out)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const UnitRanges ur = P.units[u];
    const svt_fetch_unit w = P.windows[u];
    const svt_breakpoint bp = P.bps[u];
    if (lane == 0) { S.n_reads = 0; S.n_walked = 0; S.n_rows = 0; S.status = ur.preset; S.lcp = 0; }
    X::sync();
    if (S.status == EW_OK) gather_window<X>(P, S, P.ranges + ur.first, ur.n[0], w.tid_a, w.lo_a, w.hi_a, bp.pos_a, bp.pos_b);
    X::sync();
    if (S.status == EW_OK) gather_window<X>(P, S, P.ranges + ur.first + ur.n[0], ur.n[1], w.tid_b, w.lo_b, w.hi_b, bp.pos_a, bp.pos_b);
    X::sync();
    if (S.status != EW_OK) return;
    const uint32_t n = S.n_reads;
    if (n == 0) return;

    // ---- order by (query name, arrival): the common prefix once, then eight bytes behind it as the key
    {
        uint32_t lcp = S.reads[0].name_len;
        const uint8_t* a = P.arena + S.reads[0].name_off;
        for (uint32_t k = lane; k < n; k += lanes) {
            const uint8_t* b = P.arena + S.reads[k].name_off;
            const uint32_t m = lcp < S.reads[k].name_len ? lcp : S.reads[k].name_len;
            uint32_t i = 0;
            while (i < m && a[i] == b[i]) ++i;
            lcp = i;
        }
        S.s.rows[lane] = (uint16_t)lcp;                      // (lanes() <= kMaxReads)
        X::sync();
        if (lane == 0) {
            uint32_t m = S.s.rows[0];
            for (uint32_t k = 1; k < lanes; ++k) m = S.s.rows[k] < m ? S.s.rows[k] : m;
            S.lcp = m;
        }
        X::sync();
    }
    const uint32_t lcp = S.lcp;
    for (uint32_t k = lane; k < n; k += lanes) {
        const uint8_t* p = P.arena + S.reads[k].name_off + lcp;
        const uint32_t have = S.reads[k].name_len - lcp;
        uint64_t key = 0;
        for (uint32_t i = 0; i < 8; ++i) key = (key << 8) | (i < have ? p[i] : 0u);
        S.s.key[k] = key;
    }
    X::sync();
    for (uint32_t k = lane; k < n; k += lanes) {              // rank = reads in front of this one
        const uint64_t key = S.s.key[k];
        const ReadSum& me = S.reads[k];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint64_t kj = S.s.key[j];
            bool less;
            if (kj != key) less = kj < key;
            else if (j == k) less = false;
            else {
                const int c = name_cmp(P.arena + S.reads[j].name_off, S.reads[j].name_len, P.arena + me.name_off, me.name_len);
                less = c != 0 ? c < 0 : j < k;
            }
            rank += less ? 1u : 0u;
        }
        S.s.rowoff[k] = (uint16_t)rank;
    }
    X::sync();
    for (uint32_t k = lane; k < n; k += lanes) S.s.order[S.s.rowoff[k]] = (uint16_t)k;
    X::sync();
    // ---- fragments: runs of one name; bit 15 of order[] marks the first read of a run
    for (uint32_t p = lane; p < n; p += lanes) {
        const bool first = p == 0 || !same_name(P, S.reads[S.s.order[p] & 0x7fff], S.reads[S.s.order[p - 1] & 0x7fff]);
        S.s.rows[p] = first ? 1 : 0;
    }
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes)
        if (S.s.rows[p]) S.s.order[p] |= 0x8000;
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes) {              // the same (name, flag) again: dropped
        ReadSum& me = S.reads[S.s.order[p] & 0x7fff];
        bool dup = false;
        for (uint32_t q = p; q > 0 && !(S.s.order[q] & 0x8000) && !dup;) {
            --q;
            dup = S.reads[S.s.order[q] & 0x7fff].flag == me.flag;
        }
        if (dup) me.bits |= RS_DUP;
    }
    X::sync();
    for (uint32_t p = lane; p < n; p += lanes) {              // rows of the fragment: max(1, ceil(primaries / 2), |seq|, |clip|)
        uint32_t rows = 0;
        if (S.s.order[p] & 0x8000) {
            uint32_t np = 0, ns = 0, nc = 0;
            for (uint32_t q = p; q < n && (q == p || !(S.s.order[q] & 0x8000)); ++q) {
                const ReadSum& m = S.reads[S.s.order[q] & 0x7fff];
                if (!is_primary(m)) continue;
                ++np;
                if (m.bits & RS_SPLIT) { if (m.bits & RS_SOFT) ++nc; else ++ns; }
            }
            rows = (np + 1) / 2;
            rows = rows < 1 ? 1 : rows;
            rows = rows < ns ? ns : rows;
            rows = rows < nc ? nc : rows;
        }
        S.s.rows[p] = (uint16_t)rows;
    }
    X::sync();
    if (lane == 0) {
        uint32_t at = 0;
        for (uint32_t p = 0; p < n; ++p) { S.s.rowoff[p] = (uint16_t)at; at += S.s.rows[p]; }
        S.n_rows = at;
    }
    X::sync();
    if (!out) return;
    for (uint32_t p = lane; p < n; p += lanes) {
        const uint32_t rows = S.s.rows[p];
        if (!rows) continue;
        uint32_t end = p + 1;
        while (end < n && !(S.s.order[end] & 0x8000)) ++end;
        const uint32_t lib = S.reads[S.s.order[p] & 0x7fff].lib;        // SamFragment(read, lib): the first read's
        uint32_t np = 0;
        for (uint32_t q = p; q < end; ++q) np += is_primary(S.reads[S.s.order[q] & 0x7fff]) ? 1u : 0u;
        uint32_t qp = p, qs = p, qc = p;                   // cursors: next primary / seq candidate / clip candidate
        for (uint32_t k = 0; k < rows; ++k) {
            ReadS ra = absent_read(), rb = absent_read();
            PieceS sl = absent_piece(), sr = absent_piece(), cl = absent_piece(), cr = absent_piece();
            for (int j = 0; j < 2; ++j) {
                while (qp < end && !is_primary(S.reads[S.s.order[qp] & 0x7fff])) ++qp;
                if (qp < end) { (j ? rb : ra) = read_of_sum(S.reads[S.s.order[qp] & 0x7fff]); ++qp; }
            }
            for (; qs < end; ++qs) {
                const ReadSum& m = S.reads[S.s.order[qs] & 0x7fff];
                if (is_primary(m) && (m.bits & RS_SPLIT) && !(m.bits & RS_SOFT)) { sl = piece_of_sum(m, true); sr = piece_of_sum(m, false); ++qs; break; }
            }
            for (; qc < end; ++qc) {
                const ReadSum& m = S.reads[S.s.order[qc] & 0x7fff];
                if (is_primary(m) && (m.bits & RS_SPLIT) && (m.bits & RS_SOFT)) { cl = piece_of_sum(m, true); cr = piece_of_sum(m, false); ++qc; break; }
            }
            ra.extra = lib;
            rb.extra = ((k == 0 && np == 2) ? SVT_FRAG_PAIR : 0u) | (k > 0 ? SVT_FRAG_CONTINUATION : 0u);
            out[S.s.rowoff[p] + k] = geometry_record(ra, rb, sl, sr, cl, cr, bp, P.lib_flank[lib], P.min_aligned, P.split_slop);
        }
    }
    X::sync();
}

}  // namespace ew
}  // namespace svt

#endif  // SVT_EVIDENCE_WALK_H

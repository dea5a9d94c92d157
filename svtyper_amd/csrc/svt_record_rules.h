// svt_record_rules.h -- the rules of one BAM alignment record that the split-read path rests on (the reference's
// SplitRead.is_valid and its relatives: svtyper/parsers.py:922-1058, 1062-1101, 1242-1253), stated ONCE for the host reader
// (svt_reads_fragments.h: process_unit) and the evidence walk (svt_evidence_walk.h, host and gfx950): the fixed fields of a record,
// the CIGAR operation classes, the query interval of a CIGAR, the text CIGAR and the fields of an SA entry, the tag grammar,
// the gap-free aligned intervals, and the arithmetic of a split-read candidate.
//
// Plain functions over `const uint8_t*` + length: no std::, no allocation, every access checked against the length given,
// every loop bounded by a length.  This layer does grammar and arithmetic on numbers.  What the two callers do differently
// stays with them: how the text of an SA number becomes a number, how a name becomes a tid, which limits apply (they are
// arguments here) and what a failure is called (error text there, EW_* reason here).
#ifndef SVT_RECORD_RULES_H
#define SVT_RECORD_RULES_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace rr {

// ---- bytes and numbers ------------------------------------------------------------------------------------------------------
SVT_HD uint32_t ld32(const uint8_t* d) { return (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24); }
SVT_HD int32_t clip32(int64_t x) { return (int32_t)(x < (int64_t)INT32_MIN ? (int64_t)INT32_MIN : x > (int64_t)INT32_MAX ? (int64_t)INT32_MAX : x); }
SVT_HD int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
SVT_HD int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
SVT_HD int64_t abs64(int64_t a) { return a < 0 ? -a : a; }

// ---- CIGAR ------------------------------------------------------------------------------------------------------------------
SVT_HD bool op_clip(uint32_t op) { return op == 4 || op == 5; }
SVT_HD bool op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }
SVT_HD bool op_query(uint32_t op) { return op == 0 || op == 1 || op == 7 || op == 8; }
SVT_HD bool op_aligned(uint32_t op) { return op == 0 || op == 7 || op == 8; }

// what the query interval, "left clipped" and the clip rules need of a CIGAR, gathered in one forward pass
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
// the CIGAR words of a record
SVT_HD void cigar_of_words(const uint8_t* cig, uint32_t n_cigar, CigarStats& c)
{
    cigar_begin(c);
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t w = ld32(cig + 4 * k);
        cigar_add(c, w & 0xF, (int64_t)(w >> 4));
    }
}
// a text CIGAR (of an SA entry).  A number of more than `max_digits` digits (at most 18: it has to fit 64 bits) is malformed;
// more than `max_ops` operations is the caller's limit.
enum : uint32_t { CIGAR_OK = 0, CIGAR_MALFORMED = 1, CIGAR_TOO_MANY = 2 };
SVT_HD uint32_t cigar_of_string(const uint8_t* s, uint32_t n, uint32_t max_ops, uint32_t max_digits, CigarStats& c)
{
    cigar_begin(c);
    int64_t num = 0;
    uint32_t nd = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t ch = s[i];
        if (ch >= '0' && ch <= '9') {
            if (++nd > max_digits) return CIGAR_MALFORMED;
            num = num * 10 + (ch - '0');
            continue;
        }
        uint32_t op;
        switch (ch) {
        case 'M': op = 0; break; case 'I': op = 1; break; case 'D': op = 2; break; case 'N': op = 3; break; case 'S': op = 4; break;
        case 'H': op = 5; break; case 'P': op = 6; break; case '=': op = 7; break; case 'X': op = 8; break;
        default: return CIGAR_MALFORMED;
        }
        if (nd == 0) return CIGAR_MALFORMED;
        if (c.n >= max_ops) return CIGAR_TOO_MANY;
        cigar_add(c, op, num);
        num = 0;
        nd = 0;
    }
    return nd ? CIGAR_MALFORMED : CIGAR_OK;
}

struct QPos { int64_t start, end, length; };
// the query interval: the clip met first (the last operation of a reverse read) opens the query
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

// ---- one record -----------------------------------------------------------------------------------------------------------
struct Core {
    int32_t tid, pos, l_seq;
    uint32_t l_name, n_cigar, flag, mapq, tags_off;
    int64_t end;                               // reference end: pos + the reference-consuming operations
};
// the fixed fields, the reference end and where the tags begin; false when the variable-length parts do not fit `size`.
// (l_seq is added up as the unsigned 64-bit number it becomes: a negative one passes when it moves tags_off back by less than
// what lies in front of it.  The host reader takes such a record as it then is; the walk refuses l_seq < 0 itself.)
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
    off += (uint64_t)(((int64_t)r.l_seq + 1) / 2 + (int64_t)r.l_seq);
    if (off > size) return false;
    r.tags_off = (uint32_t)off;
    return true;
}

// ---- tags -----------------------------------------------------------------------------------------------------------------
// The first RG:Z and the first SA:Z values met so far (offset into the record, length without the NUL).  One walk can be made
// in two legs: walk_tags(..., stop_at_rg = true) returns TAGS_AT_RG with `at` behind the RG value, a second call goes on from
// there with the same Tags.
struct Tags { uint32_t rg_off, rg_len, sa_off, sa_len; bool have_rg, have_sa; };
SVT_HD void tags_begin(Tags& t)
{
    t.have_rg = t.have_sa = false;
    t.rg_off = t.rg_len = t.sa_off = t.sa_len = 0;
}
enum : uint32_t {
    TAGS_END = 0,            // the whole tag area is walked
    TAGS_AT_RG = 1,          // stopped behind the first RG:Z
    TAGS_MALFORMED = 2,      // unknown type or B subtype, Z / H value without its NUL, B header cut off
    TAGS_OVERRUN = 3         // a fixed-size value or a B array that reaches beyond the record
};
SVT_HD uint32_t walk_tags(const uint8_t* d, uint32_t size, uint32_t& at, bool stop_at_rg, Tags& t)
{
    uint64_t i = at;
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
            if (q >= n) return TAGS_MALFORMED;
            skip = q - i + 1;
            if (ty == 'Z' && a0 == 'S' && a1 == 'A' && !t.have_sa) { t.have_sa = true; t.sa_off = (uint32_t)i; t.sa_len = (uint32_t)(q - i); }
            if (ty == 'Z' && a0 == 'R' && a1 == 'G' && !t.have_rg) {
                t.have_rg = true; t.rg_off = (uint32_t)i; t.rg_len = (uint32_t)(q - i);
                if (stop_at_rg) { at = (uint32_t)(i + skip); return TAGS_AT_RG; }
            }
            break;
        }
        case 'B': {
            if (i + 5 > n) return TAGS_MALFORMED;
            const uint8_t sub = d[i];
            const uint32_t cnt = ld32(d + i + 1);
            const uint64_t sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (sz == 0) return TAGS_MALFORMED;
            skip = 5 + (uint64_t)cnt * sz;
            break;
        }
        default: return TAGS_MALFORMED;
        }
        i += skip;
        if (i > n) return TAGS_OVERRUN;
    }
    return TAGS_END;
}

// One field of a tag area, by the grammar of walk_tags: the field at `at` ends at `next` (TAG_FIELD), or fewer than three
// bytes are left (TAGS_END), or the field is what walk_tags calls TAGS_MALFORMED / TAGS_OVERRUN.  For callers that need every
// field's extent (svt_dump_rules.h: the XV fields of a record).  walk_tags is not restated over it: doing so moves the register
// and spill lines of the walk and library kernels, which hold walk_tags on their hot path; that the two end alike on every
// record of the dump corpus is checked by tests/native/asan_dump_rules_main.cpp.
constexpr uint32_t TAG_FIELD = 4;
SVT_HD uint32_t tag_field(const uint8_t* d, uint32_t size, uint32_t at, uint32_t& next)
{
    uint64_t i = at;
    const uint64_t n = size;
    if (i + 3 > n) return TAGS_END;
    const uint8_t ty = d[i + 2];
    i += 3;
    uint64_t skip = 0;
    switch (ty) {
    case 'A': case 'c': case 'C': skip = 1; break;
    case 's': case 'S': skip = 2; break;
    case 'i': case 'I': case 'f': skip = 4; break;
    case 'Z': case 'H': {
        uint64_t q = i;
        while (q < n && d[q]) ++q;
        if (q >= n) return TAGS_MALFORMED;
        skip = q - i + 1;
        break;
    }
    case 'B': {
        if (i + 5 > n) return TAGS_MALFORMED;
        const uint8_t sub = d[i];
        const uint32_t cnt = ld32(d + i + 1);
        const uint64_t sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
        if (sz == 0) return TAGS_MALFORMED;
        skip = 5 + (uint64_t)cnt * sz;
        break;
    }
    default: return TAGS_MALFORMED;
    }
    i += skip;
    if (i > n) return TAGS_OVERRUN;
    next = (uint32_t)i;
    return TAG_FIELD;
}
// ---- aligned intervals ------------------------------------------------------------------------------------------------------
// The maximal gap-free aligned reference intervals of a CIGAR (geometry.aligned_intervals), reduced to what a summary keeps:
// all of them when there are at most two, else the two nearest to the breakends in the order of a stable sort by distance
// (geometry._read_words).  One pass, nothing stored but the candidates.
struct Intervals { int64_t s[2], e[2]; uint32_t n; };
SVT_HD void aligned_intervals(const uint8_t* cig, uint32_t n_cigar, int64_t pos, int64_t near_a, int64_t near_b, Intervals& out)
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
    out.n = n < 2 ? n : 2;
    out.s[0] = n > 2 ? bs[0] : fs[0];              // (what is not there is 0)
    out.e[0] = n > 2 ? be[0] : fe[0];
    out.s[1] = n > 2 ? bs[1] : fs[1];
    out.e[1] = n > 2 ? be[1] : fe[1];
}

// ---- split-read candidates ----------------------------------------------------------------------------------------------------
// A read without an SA tag is a candidate (with the dummy piece) when it is clipped at an end and at most 50 of its bases
// are not aligned.  The read is the left piece unless it is left clipped.
SVT_HD bool soft_clip_candidate(const CigarStats& a, int64_t l_seq)
{
    const bool fc = op_clip(a.first_op), lc = op_clip(a.last_op);
    if (!(fc || lc)) return false;
    const int64_t clip_length = max64(fc ? a.first_len : 0, lc ? a.last_len : 0);
    return clip_length > 0 && (l_seq - a.query) <= 50;
}

// SA:Z:chrom,pos,strand,CIGAR,mapQ,NM;...  -- the first five ','-separated fields of the value (trailing ';' stripped) as
// offsets into it and lengths; returns how many fields there are, `entries`: how many ';'-separated entries (more than one: the reference
// discards the tag).
SVT_HD uint32_t sa_fields(const uint8_t* sa, uint32_t len, uint32_t& entries, uint32_t (&off)[5], uint32_t (&flen)[5])
{
    while (len && sa[len - 1] == ';') --len;
    entries = 1;
    for (uint32_t i = 0; i < len; ++i) if (sa[i] == ';') ++entries;
    for (uint32_t k = 0; k < 5; ++k) off[k] = flen[k] = 0;
    uint32_t fields = 0, p0 = 0;
    for (uint32_t i = 0; i <= len; ++i) {
        if (i == len || sa[i] == ',') {
            if (fields < 5) { off[fields] = p0; flen[fields] = i - p0; }
            ++fields;
            p0 = i + 1;
        }
    }
    return fields;
}

// One alignment of a split read: the read itself or its SA entry.
struct Piece { int32_t tid; int64_t start, end; bool reverse; QPos q; };
// SplitRead.is_valid for a left and a right piece: at least 20 query bases of each outside the other, and on one chromosome
// and strand neither a small insertion nor a desert between them
SVT_HD bool split_valid_ordered(const Piece& l, const Piece& r)
{
    const int64_t shared = max64(0, 1 + min64(l.q.end, r.q.end) - max64(l.q.start, r.q.start));
    const int64_t non_overlap = min64(1 + l.q.end - l.q.start - shared, 1 + r.q.end - r.q.start - shared);
    if (non_overlap < 20) return false;
    if (l.tid == r.tid && l.reverse == r.reverse) {
        const int64_t l_sd = l.start - (l.reverse ? l.q.length - l.q.end : l.q.start), l_ed = l.end - (l.reverse ? l.q.length - l.q.start : l.q.end);
        const int64_t r_sd = r.start - (r.reverse ? r.q.length - r.q.end : r.q.start), r_ed = r.end - (r.reverse ? r.q.length - r.q.start : r.q.end);
        const int64_t ins = l.reverse ? r_ed - l_sd : l_ed - r_sd;
        if (abs64(ins) < 50) return false;
        const int64_t desert = r.q.start - l.q.end - 1;
        if (desert > 0 && desert - max64(0, ins) > 50) return false;
    }
    return true;
}
// ... for the read `a` and its one SA entry `b`.  `self_left`: the read is the left piece (on one chromosome the one that
// starts first, else the one that is not left clipped).
SVT_HD bool split_valid(const Piece& a, const Piece& b, bool same_chrom, bool a_left_clipped, bool& self_left)
{
    self_left = same_chrom ? !(a.start > b.start) : !a_left_clipped;
    return self_left ? split_valid_ordered(a, b) : split_valid_ordered(b, a);      // (no choice by reference: that would put the pieces into device scratch)
}

}  // namespace rr
}  // namespace svt

#endif  // SVT_RECORD_RULES_H

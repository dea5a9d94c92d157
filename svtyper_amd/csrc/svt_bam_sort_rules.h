// svt_bam_sort_rules.h -- BAM records as spans: the per-record rule of the coordinate-sorted, BAI-indexed `-w` dump (DESIGN 3.4,
// include/svtyper_reads.h: svt_bam_span).
//
// ONE piece of source for both places that run the rule, as svt_vcf_lines.h and svt_dump_rules.h are: span_of is compiled for
// the host (svt_bam_spans_host, any C++17 compiler: this is where it is proven against the restatement of tests/baicases.py and
// sanitised) and for the device (svt_bam_sort_kernel.h, one lane per record).  It reads a record's fixed part and its CIGAR
// and nothing else, every byte checked against the span the caller's offset table gives it; no std::, no allocation.  What is
// host code on both routes (the member cut of bam.BgzfWriter, the stable order's host twin) stands below it.
#ifndef SVT_BAM_SORT_RULES_H
#define SVT_BAM_SORT_RULES_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_geometry_math.h"

namespace svt {
namespace bsr {

constexpr uint64_t kBaiEnd = 1ull << 29;        // a BAI addresses [0, 2^29)
constexpr uint32_t kSaturated = 0xFFFFFFFFu;
constexpr uint32_t kFixed = 36;                 // block_size and the 32 bytes behind it

SVT_HD uint32_t ld32(const uint8_t* d) { return (uint32_t)d[0] | ((uint32_t)d[1] << 8) | ((uint32_t)d[2] << 16) | ((uint32_t)d[3] << 24); }

// the record p[0, avail) (block_size first) -> key, tid, beg, end and flags of r; off and len are the caller's
SVT_HD void span_of(const uint8_t* p, uint64_t avail, int32_t n_ref, svt_bam_span& r)
{
    r.key = 0;
    r.tid = 0;
    r.beg = r.end = 0;
    r.flags = SVT_BAM_BAD | SVT_BAM_BAD_RECORD;
    if (avail < kFixed || avail - 4 > 0x7FFFFFFFull) return;
    const uint32_t block_size = ld32(p);
    if (block_size != (uint32_t)(avail - 4)) return;
    const uint32_t l_read_name = p[12], n_cigar = (uint32_t)p[16] | (uint32_t)p[17] << 8, flag = (uint32_t)p[18] | (uint32_t)p[19] << 8;
    const uint64_t cigar_at = (uint64_t)kFixed + l_read_name;
    if (cigar_at + 4ull * n_cigar > avail) return;
    const int32_t tid = (int32_t)ld32(p + 4), pos = (int32_t)ld32(p + 8);
    r.tid = tid;
    if (tid >= n_ref || tid < -1) {
        r.flags = SVT_BAM_BAD | SVT_BAM_BAD_TID;
        return;
    }
    if (pos < -1 || (pos < 0 && tid >= 0)) {
        r.flags = SVT_BAM_BAD | SVT_BAM_BAD_POS;
        return;
    }
    r.flags = flag & 0x4 ? SVT_BAM_UNMAPPED : 0;
    const uint64_t tid_key = tid < 0 ? (uint64_t)(uint32_t)n_ref : (uint64_t)(uint32_t)tid;
    r.key = tid_key << 33 | (uint64_t)((int64_t)pos + 1) << 1 | (flag >> 4 & 1);
    if (tid < 0) {
        r.flags |= SVT_BAM_NO_COOR;
        return;
    }
    uint64_t ref_len = 0;
    if (!(flag & 0x4))
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t c = ld32(p + cigar_at + 4ull * k), op = c & 15;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;        // M D N = X
        }
    const uint64_t end = (uint64_t)(uint32_t)pos + (ref_len ? ref_len : 1);
    if (end > kBaiEnd) r.flags |= SVT_BAM_BEYOND;
    r.beg = (uint32_t)pos;
    r.end = end > kSaturated ? kSaturated : (uint32_t)end;
}

// record i of bytes[0, len) by the offset table: a span that the table does not keep inside the bytes is SVT_BAM_BAD_RECORD
SVT_HD void span_at(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t i, int32_t n_ref, svt_bam_span& r)
{
    const uint64_t at = rec_off[i], next = rec_off[i + 1];
    r.off = at;
    if (at <= next && next <= len) {
        r.len = next - at;
        span_of(bytes + at, r.len, n_ref, r);
    } else {
        r.len = 0;
        r.key = 0;
        r.tid = 0;
        r.beg = r.end = 0;
        r.flags = SVT_BAM_BAD | SVT_BAM_BAD_RECORD;
    }
}

SVT_HD uint32_t bad_kind_of(uint32_t flags)
{
    return flags & SVT_BAM_BAD_TID ? SVT_BAM_KIND_TID : flags & SVT_BAM_BAD_POS ? SVT_BAM_KIND_POS : SVT_BAM_KIND_RECORD;
}

}  // namespace bsr
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <algorithm>
#include <numeric>
#include <vector>

namespace svt {
namespace bsr {

constexpr uint64_t kPayload = 65280;            // bam.BgzfWriter's payload per member (dfl::kMaxPayload)

inline void spans_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, svt_bam_span* spans, uint64_t& key_and,
                       uint64_t& key_or)
{
    key_and = ~0ull;
    key_or = 0;
    for (uint64_t i = 0; i < n; ++i) {
        span_at(bytes, len, rec_off, i, n_ref, spans[i]);
        key_and &= spans[i].key;
        key_or |= spans[i].key;
    }
}

// the 1-based number of the first SVT_BAM_BAD span and why, or 0
inline uint64_t first_bad(const svt_bam_span* spans, uint64_t n, uint32_t& kind)
{
    kind = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (spans[i].flags & SVT_BAM_BAD) {
            kind = bad_kind_of(spans[i].flags);
            return i + 1;
        }
    return 0;
}

// svt_bam_sort_order_host without its argument checks
inline uint64_t sort_order(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint32_t& kind)
{
    if (const uint64_t bad = first_bad(spans, n, kind)) return bad;
    std::iota(perm, perm + n, (uint64_t)0);
    std::stable_sort(perm, perm + n, [&](uint64_t a, uint64_t b) { return spans[a].key < spans[b].key; });
    return 0;
}

// Where bam.BgzfWriter cuts a stream of `header_len` bytes written and flushed, then records of lens[0 .. n) handed to
// write_record, then closed: start[k] is where member k's payload begins in the stream, start.back() the stream's length.
template <typename LenAt>
inline void cut_members(uint64_t header_len, uint64_t n, LenAt len_at, std::vector<uint64_t>& start)
{
    start.clear();
    uint64_t pos = 0, buf = 0;
    auto emit = [&](uint64_t l) {
        start.push_back(pos);
        pos += l;
        buf -= l;
    };
    buf = header_len;
    while (buf >= kPayload) emit(kPayload);
    if (buf) emit(buf);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t l = len_at(i);
        if (buf && buf + l > kPayload) emit(buf);
        buf += l;
        while (buf >= kPayload) emit(kPayload);
    }
    if (buf) emit(buf);
    start.push_back(pos);
}

}  // namespace bsr
}  // namespace svt
#endif  // SVT_BAM_SORT_RULES_H

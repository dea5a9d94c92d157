// svt_bai_index.h -- the index fold of the `-w` BAM: the span table of the record stream as written (svt_bam_sort_rules.h) and
// the BGZF members that hold it -> the bytes of a .bai.  Host code, one pass over the spans; the layout is the published one
// (SAM spec 5.2: "BAI\1", n_ref, per reference its bins with their chunks, pseudo-bin 37450 and the 16 kb linear index, the
// 64-bit n_no_coor at the end; binning of SAM spec 5.3).  The fold of a reference -- chunks, linear index, pseudo-bin -- is
// tbx::Contig's (svt_tbx_index.h), the one the .tbi is made with.  Unlike the .tbi, the records are packed whole into members,
// so a position of the stream is found in the table of member starts, not by a division.
// With csi = true the same fold runs in the scheme (14, depth) whose depth is the smallest that covers l_ref_max, and the
// references are serialised as CSIv1 (svt_tbx_index.h: namespace csi, l_aux = 0); what the scheme cannot hold is decided from
// a record's end, not from its SVT_BAM_BEYOND flag.
// Byte equality with what htslib writes for the same file is not claimed.
#ifndef SVT_BAI_INDEX_H
#define SVT_BAI_INDEX_H

#include "svt_bam_sort_rules.h"
#include "svt_tbx_index.h"

namespace svt {
namespace bai {

// What the fold asks of its tables, on the host and on the device (svt_entry_bam_index.h; spans null there: the table was made by
// the call itself): null, or what is wrong with them.  member_off: where the members begin in the file, as virtual offsets can say it
inline const char* check_tables(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                                const uint64_t* member_off, uint64_t n_members)
{
    if (n_ref < 0) return "n_ref is negative";
    if (l_ref_max >> 32) return "l_ref_max is below 2^32";
    for (uint64_t k = 0; k < n_members; ++k) {
        if (member_start[k + 1] < member_start[k] || member_start[k + 1] - member_start[k] > 65536)
            return "member_start must not decrease, a member holds at most 65536 bytes";
        if (member_off[k + 1] < member_off[k] || member_off[k + 1] >> 48) return "member_off must not decrease (< 2^48)";
    }
    if (!spans) return nullptr;
    uint64_t at = n ? spans[0].off : 0;
    if (n && at < member_start[0]) return "a record lies in front of the members";
    for (uint64_t i = 0; i < n; ++i) {              // the table of a stream as written: the records side by side
        if (spans[i].off != at || spans[i].len > member_start[n_members] - at) return "the records do not tile the stream";
        at += spans[i].len;
    }
    return nullptr;
}

// svt_bai_build (include/svtyper_reads.h) without its argument checks: 0 and the bytes in `out`, or the 1-based number of the
// record the index cannot hold and why
inline uint64_t build(const svt_bam_span* spans, uint64_t n, int32_t n_ref, const uint64_t* member_start, const uint64_t* member_off, uint64_t n_members,
                      std::vector<uint8_t>& out, uint32_t& bad_kind, bool csi = false, uint64_t l_ref_max = 0)
{
    const uint32_t depth = csi ? idx::depth_for(l_ref_max) : idx::kBaiDepth;
    const uint64_t limit = idx::scheme_end(depth);
    uint64_t k = 0;                                 // the member that holds the position asked for last: positions only rise
    auto voff = [&](uint64_t x) {
        while (k < n_members && x >= member_start[k + 1]) ++k;
        return k >= n_members ? member_off[n_members] << 16 : member_off[k] << 16 | (x - member_start[k]);
    };
    std::vector<tbx::Contig> refs((size_t)n_ref);
    for (tbx::Contig& c : refs) c.depth = depth;
    uint64_t no_coor = 0, last_key = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const svt_bam_span& r = spans[i];
        if (r.flags & SVT_BAM_BAD) { bad_kind = bsr::bad_kind_of(r.flags); return i + 1; }
        if (r.key < last_key) { bad_kind = SVT_BAM_KIND_KEY_BACK; return i + 1; }
        last_key = r.key;
        if (r.flags & SVT_BAM_NO_COOR) { ++no_coor; continue; }
        if (csi ? r.end == bsr::kSaturated || r.end > limit : (r.flags & SVT_BAM_BEYOND) != 0) { bad_kind = SVT_BAM_KIND_BEYOND; return i + 1; }
        if (r.tid < 0 || r.tid >= n_ref) { bad_kind = SVT_BAM_KIND_TID; return i + 1; }
        const uint64_t beg = r.beg, end = std::max<uint64_t>(r.end, beg + 1);
        const uint64_t s = voff(r.off), e = voff(r.off + r.len);
        tbx::Contig& c = refs[(size_t)r.tid];
        c.add(beg, end, s, e);
        if (r.flags & SVT_BAM_UNMAPPED) ++c.unmapped;
    }
    tbx::Builder b;
    if (csi) {
        csi::write(b, depth, std::vector<uint8_t>(), refs, no_coor);
        out.swap(b.out);
        return 0;
    }
    b.out.assign({'B', 'A', 'I', 1});
    b.u32((uint32_t)n_ref);
    for (tbx::Contig& c : refs) c.write(b);
    b.u64(no_coor);
    out.swap(b.out);
    return 0;
}

}  // namespace bai
}  // namespace svt

#endif  // SVT_BAI_INDEX_H

// svt_bai_index.h -- the index fold of the `-w` BAM: the span table of the record stream as written (svt_bam_sort_rules.h) and
// the BGZF members that hold it -> the bytes of a .bai.  Host code, one pass over the spans; the layout is the published one
// (SAM spec 5.2: "BAI\1", n_ref, per reference its bins with their chunks, pseudo-bin 37450 and the 16 kb linear index, the
// 64-bit n_no_coor at the end; binning of SAM spec 5.3).  The fold of a reference -- chunks, linear index, pseudo-bin -- is
// tbx::Contig's (svt_tbx_index.h), the one the .tbi is made with.  Unlike the .tbi, the records are packed whole into members,
// so a position of the stream is found in the table of member starts, not by a division.
// Byte equality with what htslib writes for the same file is not claimed.
#ifndef SVT_BAI_INDEX_H
#define SVT_BAI_INDEX_H

#include "svt_bam_sort_rules.h"
#include "svt_tbx_index.h"

namespace svt {
namespace bai {

// svt_bai_build (include/svtyper_reads.h) without its argument checks: 0 and the bytes in `out`, or the 1-based number of the
// record the index cannot hold and why
inline uint64_t build(const svt_bam_span* spans, uint64_t n, int32_t n_ref, const uint64_t* member_start, const uint64_t* member_off, uint64_t n_members,
                      std::vector<uint8_t>& out, uint32_t& bad_kind)
{
    uint64_t k = 0;                                 // the member that holds the position asked for last: positions only rise
    auto voff = [&](uint64_t x) {
        while (k < n_members && x >= member_start[k + 1]) ++k;
        return k >= n_members ? member_off[n_members] << 16 : member_off[k] << 16 | (x - member_start[k]);
    };
    std::vector<tbx::Contig> refs((size_t)n_ref);
    uint64_t no_coor = 0, last_key = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const svt_bam_span& r = spans[i];
        if (r.flags & SVT_BAM_BAD) { bad_kind = bsr::bad_kind_of(r.flags); return i + 1; }
        if (r.key < last_key) { bad_kind = SVT_BAM_KIND_KEY_BACK; return i + 1; }
        last_key = r.key;
        if (r.flags & SVT_BAM_NO_COOR) { ++no_coor; continue; }
        if (r.flags & SVT_BAM_BEYOND) { bad_kind = SVT_BAM_KIND_BEYOND; return i + 1; }
        if (r.tid < 0 || r.tid >= n_ref) { bad_kind = SVT_BAM_KIND_TID; return i + 1; }
        const uint64_t beg = r.beg, end = std::max<uint64_t>(r.end, beg + 1);
        const uint64_t s = voff(r.off), e = voff(r.off + r.len);
        tbx::Contig& c = refs[(size_t)r.tid];
        c.add(beg, end, s, e);
        if (r.flags & SVT_BAM_UNMAPPED) ++c.unmapped;
    }
    tbx::Builder b;
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

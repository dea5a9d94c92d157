// svt_index_scheme.h -- the binning scheme (min_shift, depth) of the indexes this library writes: .bai and .tbi are (14, 5), a
// .csi is (14, depth) with the smallest depth >= 5 whose 2^(14 + 3 depth) covers the file (SAM spec 5.3, CSIv1).  ONE piece of
// source for the host fold (svt_tbx_index.h) and the device fold (svt_bam_index_kernel.h): integers only, no
// std::, no allocation.  min_shift is 14 always; positions are below 2^32, so depth is 5 or 6 and a bin number fits 32 bits.
#ifndef SVT_INDEX_SCHEME_H
#define SVT_INDEX_SCHEME_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace idx {

constexpr uint32_t kMinShift = 14;
constexpr uint32_t kBaiDepth = 5;
constexpr uint32_t kMaxDepth = 6;               // 2^(14 + 18) = 2^32: every position a span or a line table can carry

// the smallest depth >= 5 whose scheme covers [0, max_end)
SVT_HD uint32_t depth_for(uint64_t max_end)
{
    uint32_t d = kBaiDepth;
    while (d < 16 && (1ull << (kMinShift + 3 * d)) < max_end) ++d;
    return d;
}

// the positions the scheme addresses: [0, scheme_end)
SVT_HD uint64_t scheme_end(uint32_t depth) { return 1ull << (kMinShift + 3 * depth); }

// the first bin of level l (0 = the root)
SVT_HD uint32_t level_first(uint32_t l) { return (uint32_t)(((1ull << (3 * l)) - 1) / 7); }

// the smallest bin that holds [beg, end), end > beg
SVT_HD uint32_t reg2bin(uint64_t beg, uint64_t end, uint32_t depth)
{
    --end;
    uint32_t s = kMinShift;
    for (uint32_t l = depth; l > 0; --l, s += 3)
        if (beg >> s == end >> s) return level_first(l) + (uint32_t)(beg >> s);
    return 0;
}

// the first position of bin `bin`
SVT_HD uint64_t bin_start(uint32_t bin, uint32_t depth)
{
    uint32_t l = 0;
    while (l < depth && level_first(l + 1) <= bin) ++l;
    return (uint64_t)(bin - level_first(l)) << (kMinShift + 3 * (depth - l));
}

// the bin that carries a reference's (first start, last end) and (mapped, unmapped): 37450 at depth 5
SVT_HD uint32_t pseudo_bin(uint32_t depth) { return level_first(depth + 1) + 1; }

// What a fold leaves for the CSIv1 serialiser (svt_tbx_index.h: csi::serialise), on the host or on the device: a run of consecutive
// records with one bin -- one chunk --, and a row per reference.
struct Run { uint64_t key, s, e; };                 // records at virtual offsets [s, e) in bin (uint32_t)key of reference key >> 32
struct RefRow { uint64_t first, last, mapped, unmapped; };      // mapped + unmapped = 0: a reference without records

}  // namespace idx
}  // namespace svt

#endif  // SVT_INDEX_SCHEME_H

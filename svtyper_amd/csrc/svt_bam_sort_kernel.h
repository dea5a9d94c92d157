// svt_bam_sort_kernel.h -- svt_bam_sort_rules.h on the device (gfx950): the records of a BAM stream in HBM -> their span table
// and the (key, index) pairs that the radix sort of svt_radix_sort_kernel.h takes.
//
//   svt_bam_keys_kernel      one lane per record, from the stream and the table of record offsets: bsr::span_at writes spans[i],
//                            keys[i] and idx[i] = i; the AND and the OR of a workgroup's keys go to key_and[block] / key_or[block]
//                            (radix_store_and_or).
// The radix passes follow, and behind them the gather, which is svt_vcf_gather_kernel<svt_bam_span>.
// Every load is checked against the stream's length (bsr::span_at) or the element count, every store against the table's.
#ifndef SVT_BAM_SORT_KERNEL_H
#define SVT_BAM_SORT_KERNEL_H

#include "svt_bam_sort_rules.h"
#include "svt_radix_sort_kernel.h"

namespace svt {

__global__ __launch_bounds__(kSortBlock) void svt_bam_keys_kernel(const uint8_t* __restrict__ bytes, uint64_t len, const uint64_t* __restrict__ rec_off,
                                                                  uint64_t n, int32_t n_ref, svt_bam_span* __restrict__ spans,
                                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                  uint64_t* __restrict__ key_and, uint64_t* __restrict__ key_or)
{
    uint64_t a = ~0ull, o = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSortBlock) {
        svt_bam_span r;
        bsr::span_at(bytes, len, rec_off, i, n_ref, r);       // (rec_off holds n + 1 entries: i + 1 <= n)
        spans[i] = r;
        keys[i] = r.key;
        idx[i] = (uint32_t)i;
        a &= r.key;
        o |= r.key;
    }
    radix_store_and_or(a, o, key_and, key_or);
}

}  // namespace svt

#endif  // SVT_BAM_SORT_KERNEL_H

// svt_bam_first_kernel.h -- svt_bam_first_rules.h on the device (gfx950): which records of a BAM stream in HBM are the first with
// their key (query name, flag).
//
//   svt_bam_first_hash_kernel  one lane per record, from the stream and the table of record offsets: bfr::key_at checks the record
//                              and reads its key, keys[i] = key_hash & mask, idx[i] = i; a record that is not well-formed goes
//                              into *bad as the smallest such index (one 64-bit atomic minimum) and hashes to 0.  The AND and the
//                              OR of a workgroup's hashes go to key_and[block] / key_or[block] (radix_store_and_or).
//   the radix passes of svt_radix_sort_kernel.h over (hash, index), as they are: stable, so inside a run of equal hashes the
//   indices rise
//   svt_bam_first_mark_kernel  one lane per sorted position j, i = idx[j]: it walks back over idx[j - 1], idx[j - 2], ... while
//                              their hash is its own, and stops at the first whose key is equal: keep[i] = 0.  At the start of
//                              the run without a hit: keep[i] = 1.  Everything in front of j in its run is earlier in the
//                              caller's order, and equal keys have equal hashes, so this is "no j' < i has i's key".  A run of one
//                              key ends at the first step; only distinct keys with one hash cost more.  A workgroup's count of
//                              kept records (ballots, then LDS across the four waves) goes to kept[block]: the host sums them.
// Every load of the stream goes through bfr::key_at (the record's own span), every index that came out of the sort is checked
// against n before it is used, every store against the element count.
#ifndef SVT_BAM_FIRST_KERNEL_H
#define SVT_BAM_FIRST_KERNEL_H

#include "svt_bam_first_rules.h"
#include "svt_radix_sort_kernel.h"

namespace svt {

constexpr unsigned long long kFirstNoBad = ~0ull;

__global__ __launch_bounds__(kSortBlock) void svt_bam_first_hash_kernel(const uint8_t* __restrict__ bytes, uint64_t len, const uint64_t* __restrict__ rec_off,
                                                                        uint64_t n, uint64_t mask, uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                        uint64_t* __restrict__ key_and, uint64_t* __restrict__ key_or,
                                                                        unsigned long long* __restrict__ bad)
{
    uint64_t a = ~0ull, o = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSortBlock) {
        bfr::Key k;
        uint64_t h = 0;
        if (bfr::key_at(bytes, len, rec_off, i, k)) h = bfr::key_hash(k) & mask;       // (rec_off holds n + 1 entries: i + 1 <= n)
        else atomicMin(bad, (unsigned long long)i);
        keys[i] = h;
        idx[i] = (uint32_t)i;
        a &= h;
        o |= h;
    }
    radix_store_and_or(a, o, key_and, key_or);
}

// keys / idx: the (hash, index) pairs in stable order by hash
__global__ __launch_bounds__(kSortBlock) void svt_bam_first_mark_kernel(const uint8_t* __restrict__ bytes, uint64_t len, const uint64_t* __restrict__ rec_off,
                                                                        uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                                        uint8_t* __restrict__ keep, uint32_t* __restrict__ kept)
{
    __shared__ uint32_t part[kSortWaves];
    uint32_t mine = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kSortBlock) {
        const uint64_t i = idx[j];
        bfr::Key k;
        if (i >= n || !bfr::key_at(bytes, len, rec_off, i, k)) continue;      // (the hash kernel found every record well-formed)
        const uint64_t h = keys[j];
        bool first = true;
        for (uint64_t b = j; b > 0 && keys[b - 1] == h; --b) {
            const uint64_t e = idx[b - 1];
            bfr::Key earlier;
            if (e < n && bfr::key_at(bytes, len, rec_off, e, earlier) && bfr::key_equal(k, earlier)) {
                first = false;
                break;
            }
        }
        keep[i] = first ? 1 : 0;
        mine += first ? 1u : 0u;
    }
    for (int d = 32; d; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d);    // (behind the loop: every lane is here)
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kSortWaves; ++w) mine += part[w];
        kept[blockIdx.x] = mine;
    }
}

}  // namespace svt

#endif  // SVT_BAM_FIRST_KERNEL_H

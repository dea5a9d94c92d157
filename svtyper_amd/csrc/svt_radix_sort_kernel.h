// svt_radix_sort_kernel.h -- a stable LSD radix sort of (64-bit key, 32-bit index) pairs in HBM with 8-bit digits (gfx950).  It
// knows nothing of what the keys are: the record sort (svt_bam_sort_kernel.h), the first-occurrence pass (svt_bam_first_kernel.h)
// and the index fold's run sort (svt_bam_index_kernel.h) each write keys and indices with a kernel of their own, which ends in
// radix_store_and_or; the host side is RadixSort (svt_entry_radix_sort.h).
//
//   radix_store_and_or       what a key kernel ends in: the AND and the OR of a workgroup's keys (shuffles, then LDS across the
//                            four waves) go to key_and[block] / key_or[block].  The host combines them: an 8-bit digit in which
//                            all keys agree is skipped.
//   per remaining digit, least significant first, over tiles of kSortTile = 1024 elements (a workgroup; wave w holds elements
//   256 w .. 256 w + 255 of it, four rounds of 64):
//   svt_bam_histogram_kernel the tile's count per digit value, hist[value * n_tiles + tile] (value-major: one exclusive scan of
//                            the whole array is where (value, tile) begins in the output)
//   svt_bam_scan_kernel      that exclusive scan, one workgroup: a lane sums a contiguous piece, the 256 sums are scanned in LDS
//   svt_bam_scatter_kernel   the tile again: 256 counters per wave in LDS, first the wave's counts, then (lane = digit value)
//                            turned into where the wave's first element of each value goes; a round of 64 keys is ranked by
//                            wave64 ballots on the digit's eight bits -- the lanes with my value that stand below me --, stored,
//                            and the value's last lane moves the counter on.
// Where an element goes is a rank: the counts are sums, the sums are scanned in a fixed order, and nothing is claimed with a
// global atomic, so the permutation is a function of the keys alone and equal keys keep their order.  (The LDS adds of the
// counting phases are integer sums: their order does not show.)  Every load is checked against the element count, every store
// against the table's.  The tile constants are also the tile geometry of svt_bam_index_kernel.h's scan.
#ifndef SVT_RADIX_SORT_KERNEL_H
#define SVT_RADIX_SORT_KERNEL_H

#include <cstdint>

namespace svt {

constexpr int kSortBlock = 256;                     // four wavefronts
constexpr uint32_t kSortWaves = kSortBlock / 64;
constexpr uint32_t kSortRounds = 4;                 // rounds of 64 elements per wave
constexpr uint32_t kSortTile = kSortBlock * kSortRounds;

// a lane's AND and OR of its keys -> the workgroup's, in key_and[blockIdx.x] / key_or[blockIdx.x].  Behind the key kernel's loop:
// every lane of the workgroup (kSortBlock of them) is here
__device__ inline void radix_store_and_or(uint64_t a, uint64_t o, uint64_t* __restrict__ key_and, uint64_t* __restrict__ key_or)
{
    __shared__ uint64_t part_and[kSortWaves], part_or[kSortWaves];
    for (int d = 32; d; d >>= 1) {
        a &= (uint64_t)__shfl_xor((unsigned long long)a, d);
        o |= (uint64_t)__shfl_xor((unsigned long long)o, d);
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part_and[wave] = a;
        part_or[wave] = o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kSortWaves; ++w) {
            a &= part_and[w];
            o |= part_or[w];
        }
        key_and[blockIdx.x] = a;
        key_or[blockIdx.x] = o;
    }
}

// hist[value * n_tiles + tile]: how many of the tile's keys have `value` in the digit at `shift`
__global__ __launch_bounds__(kSortBlock) void svt_bam_histogram_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t n_tiles, uint32_t shift,
                                                                       uint32_t* __restrict__ hist)
{
    __shared__ uint32_t count[256];
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        count[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t r = 0; r < kSortRounds; ++r) {
            const uint64_t i = (uint64_t)t * kSortTile + r * kSortBlock + threadIdx.x;
            if (i < n) atomicAdd(&count[(uint32_t)(keys[i] >> shift) & 255u], 1u);
        }
        __syncthreads();
        hist[(uint64_t)threadIdx.x * n_tiles + t] = count[threadIdx.x];
        __syncthreads();
    }
}

// hist[0, m) -> its exclusive prefix sums, in place; ONE workgroup
__global__ __launch_bounds__(kSortBlock) void svt_bam_scan_kernel(uint32_t* __restrict__ hist, uint64_t m)
{
    __shared__ uint32_t sums[kSortBlock];
    const uint64_t piece = (m + kSortBlock - 1) / kSortBlock;
    const uint64_t lo = piece * threadIdx.x < m ? piece * threadIdx.x : m, hi = lo + piece < m ? lo + piece : m;
    uint32_t s = 0;
    for (uint64_t i = lo; i < hi; ++i) s += hist[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {                         // (256 additions: not worth a tree)
        uint32_t run = 0;
        for (uint32_t k = 0; k < kSortBlock; ++k) {
            const uint32_t v = sums[k];
            sums[k] = run;
            run += v;
        }
    }
    __syncthreads();
    uint32_t run = sums[threadIdx.x];
    for (uint64_t i = lo; i < hi; ++i) {
        const uint32_t v = hist[i];
        hist[i] = run;
        run += v;
    }
}

// (keys, idx) -> (keys_out, idx_out) in stable order by the digit at `shift`; start = the scanned histogram
__global__ __launch_bounds__(kSortBlock) void svt_bam_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n,
                                                                     uint32_t n_tiles, uint32_t shift, const uint32_t* __restrict__ start,
                                                                     uint64_t* __restrict__ keys_out, uint32_t* __restrict__ idx_out)
{
    __shared__ uint32_t counter[kSortWaves][256];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        for (uint32_t w = 0; w < kSortWaves; ++w) counter[w][threadIdx.x] = 0;
        __syncthreads();
        uint64_t key[kSortRounds];
        uint32_t from[kSortRounds];
        const uint64_t first = (uint64_t)t * kSortTile + (uint64_t)wave * (64 * kSortRounds) + lane;
        for (uint32_t r = 0; r < kSortRounds; ++r) {
            const uint64_t i = first + r * 64;
            key[r] = 0;
            from[r] = 0;
            if (i < n) {
                key[r] = keys[i];
                from[r] = idx[i];
                atomicAdd(&counter[wave][(uint32_t)(key[r] >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        {                                           // lane = digit value: the waves' counts -> where each wave's first one goes
            uint32_t at = start[(uint64_t)threadIdx.x * n_tiles + t];
            for (uint32_t w = 0; w < kSortWaves; ++w) {
                const uint32_t c = counter[w][threadIdx.x];
                counter[w][threadIdx.x] = at;
                at += c;
            }
        }
        __syncthreads();
        for (uint32_t r = 0; r < kSortRounds; ++r) {    // (every lane takes every round: the ballots and barriers are everybody's)
            const bool have = first + r * 64 < n;
            const uint32_t digit = (uint32_t)(key[r] >> shift) & 255u;
            unsigned long long peers = __ballot(have);
            for (uint32_t b = 0; b < 8; ++b) {
                const unsigned long long set = __ballot((digit >> b) & 1u);
                peers &= (digit >> b) & 1u ? set : ~set;
            }
            const uint32_t base = have ? counter[wave][digit] : 0;
            const uint32_t rank = (uint32_t)__popcll(peers & below);
            __syncthreads();
            if (have) {
                const uint64_t to = (uint64_t)base + rank;
                if (to < n) {
                    keys_out[to] = key[r];
                    idx_out[to] = from[r];
                }
                if ((peers >> lane) >> 1 == 0) counter[wave][digit] = base + (uint32_t)__popcll(peers);    // the value's last lane
            }
            __syncthreads();
        }
    }
}

}  // namespace svt

#endif  // SVT_RADIX_SORT_KERNEL_H

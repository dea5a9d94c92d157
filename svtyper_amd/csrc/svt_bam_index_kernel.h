// svt_bam_index_kernel.h -- the index fold of the `-w` BAM on the device (gfx950): the span table of the record stream as written
// and the BGZF members that hold it -> the runs, loffsets and per-reference rows the CSIv1 serialiser takes (svt_tbx_index.h:
// csi::serialise; svt_index_scheme.h: idx::Run, idx::RefRow).  The record written j-th is spans[perm[j]] lying at dst_off[j] of
// the written stream (perm / dst_off null: spans[j] at spans[j].off).
//
//   svt_bam_index_record_kernel     one lane per j: s_j = the virtual offset of the record's start (a bounded binary search in
//                                   member_start), key_j = tid << 32 | bin at the scheme's depth (idx::reg2bin, the host fold's),
//                                   M_j = tid << 32 | end, and a flag byte: head (j = 0 or key_j differs from key_{j-1}, which is
//                                   recomputed, not awaited), unmapped, placed.  A record without coordinate is not placed: it is
//                                   counted (one integer add per wavefront) and keeps M = 0.  The first record the index cannot
//                                   hold and why -- SVT_BAM_BAD, a key below the key in front, beyond the scheme, a tid that is
//                                   none -- goes into ONE 64-bit integer minimum of (j + 1) << 8 | kind: the result does not
//                                   depend on the order of arrival.
//   one three-phase scan over tiles of kSortTile = 1024 records (a workgroup; a lane holds four consecutive ones), carrying the
//   sum of head, the sum of unmapped and the maximum of M together.  tid does not fall, so the plain 64-bit maximum of M is the
//   running maximum of `end` inside the reference: no segmented operator.
//   svt_bam_index_partials_kernel   a tile's three partials (shuffles, then LDS across the four waves)
//   svt_bam_index_tiles_kernel      ONE workgroup over the tile partials, the shape of svt_bam_scan_kernel: exclusive per tile, the
//                                   totals behind them
//   svt_bam_index_apply_kernel      the tile again: M becomes its inclusive running maximum, unm[j] the inclusive count of unmapped
//                                   records; a head whose exclusive count is r writes run r -- run_key[r], run_s[r] -- and ends
//                                   run r - 1 at its own start (the records lie side by side); the first record that is not
//                                   placed ends the last run, or the last record does at the end of the data.
//   No workgroup waits for another one anywhere: three launches, no look-back, no spin.
//   svt_bam_index_run_keys_kernel   idx[r] = r and the AND / OR of a workgroup's run keys (radix_store_and_or): the radix passes
//                                   of svt_radix_sort_kernel.h then sort (key, r), skipping the digits in which all keys agree
//   svt_bam_index_loffset_kernel    one lane per sorted run q: the run (key, s, e) gathered through the sorted indices; for a group
//                                   head -- a run whose key differs from the sorted run in front -- loffset = s_j for the first j
//                                   with M_j > tid << 32 | bin_start(bin), a bounded binary search over the monotone M (one
//                                   exists: the bin's own first record)
//   svt_bam_index_reference_kernel  one lane per reference: its records [lo, hi) by two binary searches in M, mapped / unmapped
//                                   from the difference of the prefix sums, first start and last end from the range
// Integers only.  Every load is checked against the element count or the member count, every store against its table's size;
// LDS holds tile partials only; the atomics are one integer min and one integer add, functions of the inputs alone.
#ifndef SVT_BAM_INDEX_KERNEL_H
#define SVT_BAM_INDEX_KERNEL_H

#include "svt_bam_sort_rules.h"
#include "svt_radix_sort_kernel.h"
#include "svt_index_scheme.h"

namespace svt {

constexpr uint8_t kIdxHead = 1, kIdxUnmapped = 2, kIdxPlaced = 4;
constexpr uint64_t kIdxNone = ~0ull;

// what the fold knows of the stream as written; n_placed (the records in front of the tail without coordinate) is set by the
// host between the scan and the searches
struct BamIndexArgs {
    const svt_bam_span* spans;
    const uint64_t* perm;           // null: the table is in written order
    const uint64_t* dst_off;        // null: spans[j].off
    uint64_t n;
    int32_t n_ref;
    uint32_t depth;
    const uint64_t* member_start;   // n_members + 1
    const uint64_t* member_off;     // n_members + 1
    uint64_t n_members;
};

// the virtual offset of stream position x: in the last member that begins at or in front of x; the end of the members behind the last
__device__ inline uint64_t idx_voff(const BamIndexArgs& a, uint64_t x)
{
    uint64_t lo = 0, hi = a.n_members + 1;          // the entries of member_start at or below x: [0, lo)
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;    // (mid <= n_members)
        if (a.member_start[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t k = lo ? lo - 1 : 0;
    if (k >= a.n_members) return a.member_off[a.n_members] << 16;
    const uint64_t in = x >= a.member_start[k] ? x - a.member_start[k] : 0;
    return a.member_off[k] << 16 | (in & 0xFFFF);
}

// the span of the record written j-th (j < n), its off where it lies in the written stream; false: perm[j] is no record
__device__ inline bool idx_span(const BamIndexArgs& a, uint64_t j, svt_bam_span& r)
{
    const uint64_t i = a.perm ? a.perm[j] : j;
    if (i >= a.n) return false;
    r = a.spans[i];
    if (a.dst_off) r.off = a.dst_off[j];
    return true;
}

// 0, or why the index cannot hold r standing behind a record with key `key_front` (SVT_BAM_KIND_*)
__device__ inline uint32_t idx_refusal(const svt_bam_span& r, bool have_front, uint64_t key_front, int32_t n_ref, uint64_t limit)
{
    if (r.flags & SVT_BAM_BAD) return bsr::bad_kind_of(r.flags);
    if (have_front && r.key < key_front) return SVT_BAM_KIND_KEY_BACK;
    if (r.flags & SVT_BAM_NO_COOR) return 0;
    if (r.end == bsr::kSaturated || r.end > limit) return SVT_BAM_KIND_BEYOND;
    if (r.tid < 0 || r.tid >= n_ref) return SVT_BAM_KIND_TID;
    return 0;
}

__device__ inline bool idx_placed(const svt_bam_span& r, int32_t n_ref, uint64_t limit)
{
    return !(r.flags & (SVT_BAM_BAD | SVT_BAM_NO_COOR)) && r.tid >= 0 && r.tid < n_ref && r.end != bsr::kSaturated && r.end <= limit;
}

__device__ inline uint64_t idx_key(const svt_bam_span& r, uint32_t depth)
{
    const uint64_t beg = r.beg, end = r.end > r.beg ? r.end : (uint64_t)r.beg + 1;
    return (uint64_t)(uint32_t)r.tid << 32 | idx::reg2bin(beg, end, depth);
}

__global__ __launch_bounds__(kSortBlock) void svt_bam_index_record_kernel(const BamIndexArgs a, uint64_t* __restrict__ s, uint64_t* __restrict__ m,
                                                                          uint64_t* __restrict__ rkey, uint8_t* __restrict__ flag,
                                                                          unsigned long long* __restrict__ first_bad,
                                                                          unsigned long long* __restrict__ no_coor)
{
    const uint64_t limit = idx::scheme_end(a.depth);
    const uint64_t rounds = (a.n + (uint64_t)gridDim.x * kSortBlock - 1) / ((uint64_t)gridDim.x * kSortBlock);
    for (uint64_t round = 0; round < rounds; ++round) {     // (every lane takes every round: the ballot is the wavefront's)
        const uint64_t j = (round * gridDim.x + blockIdx.x) * kSortBlock + threadIdx.x;
        bool counted = false;
        if (j < a.n) {
            svt_bam_span r, front;
            uint64_t sj = 0, mj = 0, kj = kIdxNone;
            uint8_t f = 0;
            uint32_t why = SVT_BAM_KIND_RECORD;
            if (idx_span(a, j, r)) {
                const bool have_front = j > 0 && idx_span(a, j - 1, front);
                why = idx_refusal(r, have_front, have_front ? front.key : 0, a.n_ref, limit);
                sj = idx_voff(a, r.off);
                counted = !why && (r.flags & SVT_BAM_NO_COOR);
                if (idx_placed(r, a.n_ref, limit)) {
                    kj = idx_key(r, a.depth);
                    mj = (uint64_t)(uint32_t)r.tid << 32 | (r.end > r.beg ? r.end : r.beg + 1);
                    const bool same = have_front && idx_placed(front, a.n_ref, limit) && idx_key(front, a.depth) == kj;
                    f = kIdxPlaced | (same ? 0 : kIdxHead) | (r.flags & SVT_BAM_UNMAPPED ? kIdxUnmapped : 0);
                }
            }
            if (why) atomicMin(first_bad, (unsigned long long)((j + 1) << 8 | why));
            s[j] = sj;
            m[j] = mj;
            rkey[j] = kj;
            flag[j] = f;
        }
        const unsigned long long tail = __ballot(counted);
        if ((threadIdx.x & 63) == 0 && tail) atomicAdd(no_coor, (unsigned long long)__popcll(tail));
    }
}

struct IdxCarry {
    uint32_t heads, unmapped;
    uint64_t top;
};

__device__ inline IdxCarry idx_join(const IdxCarry& front, const IdxCarry& back)
{
    return IdxCarry{front.heads + back.heads, front.unmapped + back.unmapped, front.top > back.top ? front.top : back.top};
}

// the four records of lane `threadIdx.x` of tile t: their carries one by one into c[], joined into the return value
__device__ inline IdxCarry idx_load4(const uint64_t* m, const uint8_t* flag, uint64_t n, uint64_t first, IdxCarry c[4])
{
    IdxCarry all{0, 0, 0};
    for (uint32_t k = 0; k < kSortRounds; ++k) {
        const uint64_t j = first + k;
        c[k] = IdxCarry{0, 0, 0};
        if (j < n) {
            const uint8_t f = flag[j];
            c[k] = IdxCarry{(uint32_t)(f & kIdxHead ? 1 : 0), (uint32_t)(f & kIdxUnmapped ? 1 : 0), m[j]};
        }
        all = idx_join(all, c[k]);
    }
    return all;
}

// tile_*[t]: the three partials of tile t
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_partials_kernel(const uint64_t* __restrict__ m, const uint8_t* __restrict__ flag, uint64_t n,
                                                                            uint32_t n_tiles, uint32_t* __restrict__ tile_heads,
                                                                            uint32_t* __restrict__ tile_unmapped, uint64_t* __restrict__ tile_top)
{
    __shared__ IdxCarry part[kSortWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        IdxCarry c[kSortRounds];
        IdxCarry mine = idx_load4(m, flag, n, (uint64_t)t * kSortTile + (uint64_t)threadIdx.x * kSortRounds, c);
        for (int d = 32; d; d >>= 1) {
            mine.heads += (uint32_t)__shfl_xor((int)mine.heads, d);
            mine.unmapped += (uint32_t)__shfl_xor((int)mine.unmapped, d);
            const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)mine.top, d);
            mine.top = mine.top > other ? mine.top : other;
        }
        if (lane == 0) part[wave] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            IdxCarry all = part[0];
            for (uint32_t w = 1; w < kSortWaves; ++w) all = idx_join(all, part[w]);
            tile_heads[t] = all.heads;
            tile_unmapped[t] = all.unmapped;
            tile_top[t] = all.top;
        }
        __syncthreads();
    }
}

// the tile partials -> what stands in front of each tile (exclusive), in place; totals[0] = all heads, totals[1] = all unmapped.
// ONE workgroup: a lane joins a contiguous piece, the 256 pieces are scanned in LDS by one lane
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_tiles_kernel(uint32_t* __restrict__ tile_heads, uint32_t* __restrict__ tile_unmapped,
                                                                         uint64_t* __restrict__ tile_top, uint32_t n_tiles, uint64_t* __restrict__ totals)
{
    __shared__ IdxCarry sums[kSortBlock];
    const uint32_t piece = (n_tiles + kSortBlock - 1) / kSortBlock;
    const uint32_t lo = (uint64_t)piece * threadIdx.x < n_tiles ? piece * threadIdx.x : n_tiles, hi = lo + piece < n_tiles ? lo + piece : n_tiles;
    IdxCarry mine{0, 0, 0};
    for (uint32_t t = lo; t < hi; ++t) mine = idx_join(mine, IdxCarry{tile_heads[t], tile_unmapped[t], tile_top[t]});
    sums[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {                         // (256 joins: not worth a tree)
        IdxCarry run{0, 0, 0};
        for (uint32_t k = 0; k < kSortBlock; ++k) {
            const IdxCarry v = sums[k];
            sums[k] = run;
            run = idx_join(run, v);
        }
        totals[0] = run.heads;
        totals[1] = run.unmapped;
    }
    __syncthreads();
    IdxCarry run = sums[threadIdx.x];
    for (uint32_t t = lo; t < hi; ++t) {
        const IdxCarry v{tile_heads[t], tile_unmapped[t], tile_top[t]};
        tile_heads[t] = run.heads;
        tile_unmapped[t] = run.unmapped;
        tile_top[t] = run.top;
        run = idx_join(run, v);
    }
}

// m -> its inclusive running maximum, unm[j] = the unmapped records among [0, j]; the runs: run_key / run_s / run_e [0, run_capacity)
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_apply_kernel(uint64_t* __restrict__ m, const uint8_t* __restrict__ flag,
                                                                         const uint64_t* __restrict__ s, const uint64_t* __restrict__ rkey, uint64_t n,
                                                                         uint32_t n_tiles, const uint32_t* __restrict__ tile_heads,
                                                                         const uint32_t* __restrict__ tile_unmapped, const uint64_t* __restrict__ tile_top,
                                                                         uint64_t end_voff, uint32_t* __restrict__ unm, uint64_t* __restrict__ run_key,
                                                                         uint64_t* __restrict__ run_s, uint64_t* __restrict__ run_e, uint64_t run_capacity)
{
    __shared__ IdxCarry part[kSortWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t first = (uint64_t)t * kSortTile + (uint64_t)threadIdx.x * kSortRounds;
        IdxCarry c[kSortRounds];
        const IdxCarry mine = idx_load4(m, flag, n, first, c);
        IdxCarry scan = mine;                       // inclusive over the wavefront's lanes
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t h = (uint32_t)__shfl_up((int)scan.heads, d), u = (uint32_t)__shfl_up((int)scan.unmapped, d);
            const uint64_t top = (uint64_t)__shfl_up((unsigned long long)scan.top, d);
            if (lane >= (uint32_t)d) scan = idx_join(IdxCarry{h, u, top}, scan);
        }
        if (lane == 63) part[wave] = scan;
        __syncthreads();
        IdxCarry front{tile_heads[t], tile_unmapped[t], tile_top[t]};       // what stands in front of this lane's four records
        for (uint32_t w = 0; w < wave; ++w) front = idx_join(front, part[w]);
        {
            const uint32_t h = (uint32_t)__shfl_up((int)scan.heads, 1), u = (uint32_t)__shfl_up((int)scan.unmapped, 1);
            const uint64_t top = (uint64_t)__shfl_up((unsigned long long)scan.top, 1);
            if (lane) front = idx_join(front, IdxCarry{h, u, top});
        }
        for (uint32_t k = 0; k < kSortRounds; ++k) {
            const uint64_t j = first + k;
            if (j >= n) break;
            const uint32_t r = front.heads;         // the heads in front of j: a head's run number
            const uint8_t f = flag[j];
            front = idx_join(front, c[k]);
            m[j] = front.top;
            unm[j] = front.unmapped;
            if (f & kIdxHead) {
                if (r < run_capacity) {
                    run_key[r] = rkey[j];
                    run_s[r] = s[j];
                }
                if (r > 0 && (uint64_t)r - 1 < run_capacity) run_e[r - 1] = s[j];
            } else if (!(f & kIdxPlaced) && j > 0 && (flag[j - 1] & kIdxPlaced)) {
                if (r > 0 && (uint64_t)r - 1 < run_capacity) run_e[r - 1] = s[j];      // the tail without coordinate begins here
            }
            if (j == n - 1 && (f & kIdxPlaced) && front.heads > 0 && (uint64_t)front.heads - 1 < run_capacity) run_e[front.heads - 1] = end_voff;
        }
        __syncthreads();
    }
}

// idx[r] = r; the AND and the OR of a workgroup's run keys
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_run_keys_kernel(const uint64_t* __restrict__ run_key, uint64_t n_runs, uint32_t* __restrict__ idx,
                                                                            uint64_t* __restrict__ key_and, uint64_t* __restrict__ key_or)
{
    uint64_t a = ~0ull, o = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; r < n_runs; r += (uint64_t)gridDim.x * kSortBlock) {
        idx[r] = (uint32_t)r;
        a &= run_key[r];
        o |= run_key[r];
    }
    radix_store_and_or(a, o, key_and, key_or);
}

// the first j in [0, n) with m[j] > target, n where there is none; m does not fall
__device__ inline uint64_t idx_first_above(const uint64_t* m, uint64_t n, uint64_t target)
{
    uint64_t lo = 0, hi = n;
    for (int step = 0; step < 64 && lo < hi; ++step) {
        const uint64_t mid = lo + (hi - lo) / 2;    // (mid < n)
        if (m[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// sorted run q: out[q] = (key, s, e) of run sorted_idx[q]; loff[q] for a group head, 0 otherwise.  m[0, n_placed): the running maximum
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_loffset_kernel(const uint64_t* __restrict__ sorted_key, const uint32_t* __restrict__ sorted_idx,
                                                                           uint64_t n_runs, const uint64_t* __restrict__ run_s,
                                                                           const uint64_t* __restrict__ run_e, const uint64_t* __restrict__ m,
                                                                           const uint64_t* __restrict__ s, uint64_t n_placed, uint32_t depth,
                                                                           idx::Run* __restrict__ out, uint64_t* __restrict__ loff)
{
    for (uint64_t q = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; q < n_runs; q += (uint64_t)gridDim.x * kSortBlock) {
        const uint64_t key = sorted_key[q];
        const uint32_t r = sorted_idx[q];
        idx::Run run{key, kIdxNone, 0};             // (s > e: what the host refuses)
        if (r < n_runs) {
            run.s = run_s[r];
            run.e = run_e[r];
        }
        uint64_t l = 0;
        if (q == 0 || sorted_key[q - 1] != key) {
            const uint64_t j = idx_first_above(m, n_placed, (key >> 32) << 32 | idx::bin_start((uint32_t)key, depth));
            l = j < n_placed ? s[j] : kIdxNone;
        }
        out[q] = run;
        loff[q] = l;
    }
}

// rows[tid]: (first start, last end, mapped, unmapped) of the records [lo, hi) whose M carries tid; zeros for a reference without records
__global__ __launch_bounds__(kSortBlock) void svt_bam_index_reference_kernel(const uint64_t* __restrict__ m, const uint64_t* __restrict__ s,
                                                                             const uint32_t* __restrict__ unm, uint64_t n, uint64_t n_placed,
                                                                             uint64_t n_ref, uint64_t end_voff, idx::RefRow* __restrict__ rows)
{
    for (uint64_t tid = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; tid < n_ref; tid += (uint64_t)gridDim.x * kSortBlock) {
        idx::RefRow row{0, 0, 0, 0};
        const uint64_t lo = idx_first_above(m, n_placed, tid << 32), hi = idx_first_above(m, n_placed, (tid + 1) << 32);    // (an end is 1 at least)
        if (lo < hi && hi <= n_placed && n_placed <= n) {
            const uint64_t unmapped = (uint64_t)unm[hi - 1] - (lo ? unm[lo - 1] : 0);
            row = idx::RefRow{s[lo], hi < n ? s[hi] : end_voff, hi - lo - unmapped, unmapped};
        }
        rows[tid] = row;
    }
}

}  // namespace svt

#endif  // SVT_BAM_INDEX_KERNEL_H

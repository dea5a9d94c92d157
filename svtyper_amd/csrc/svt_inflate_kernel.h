// svt_inflate_kernel.h -- svt_inflate.h on the device (gfx950): compressed BGZF members in HBM -> their inflated bytes in HBM.
//
// One wavefront (a workgroup of 64 lanes) per member: a member is an independent deflate stream of at most 64 KiB, a call has
// thousands of them, and that is where the parallelism is -- inside a member the bit stream is one serial chain (lane 0's), the
// other 63 lanes stage its input, build the fast decode tables, and emit each batch of symbols (svt_inflate.h has the split).
//
// Ordering of a match's loads behind the stores they read.  The output is written to HBM with ordinary byte stores and a match
// reads bytes another lane of this wave stored a moment ago: there is no window in LDS (32 KiB per wave would put LDS, not
// registers, in charge of occupancy).  X::sync() is __syncthreads(): in a one-wave workgroup the barrier itself costs nothing,
// what it brings is its workgroup-scope release / acquire fence -- the wave's stores are waited for (vmcnt) before any lane's
// later loads are issued, and the lanes of one workgroup share the CU's L1, so those loads see the stored bytes.  svt_inflate.h
// asks for it once behind a batch's literals, behind the batch, and in front of exactly those matches whose source a match of
// the same batch has written.
//
// LDS: inf::Scratch, 6 312 bytes per wave, static -- 25 waves per CU by LDS (160 KiB), more than the 8 per SIMD the registers
// allow at most: occupancy is bounded by registers (profiles/inflate_kernel_resources.txt), not by LDS.
// Everything is written with ordinary vector stores from plain C++.
#ifndef SVT_INFLATE_KERNEL_H
#define SVT_INFLATE_KERNEL_H

#include "svt_inflate.h"

namespace svt {

constexpr int kInflateBlock = 64;

struct InflateDevCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kInflateBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

// member k of `members` (payload at src + members[k].src) -> dst + members[k].dst; status[k] = inf::INF_*
__global__ __launch_bounds__(kInflateBlock) void svt_inflate_kernel(const uint8_t* __restrict__ src, uint64_t src_len, const inf::Member* __restrict__ members,
                                                                    uint32_t n, uint8_t* dst, uint64_t dst_len, uint32_t* __restrict__ status)
{
    __shared__ inf::Scratch S;
    const uint32_t k = blockIdx.x;
    if (k >= n) return;
    const inf::Member m = members[k];
    uint32_t st = inf::INF_MEMBER;                          // (every decision up to here is the same for all lanes)
    if (m.isize <= inf::kMaxIsize && m.src <= src_len && m.clen <= src_len - m.src && m.dst <= dst_len && m.isize <= dst_len - m.dst)
        st = inf::inflate_member<InflateDevCtx>(src + m.src, m.clen, dst + m.dst, m.isize, S);
    if (threadIdx.x == 0) status[k] = st;
}

}  // namespace svt

#endif  // SVT_INFLATE_KERNEL_H

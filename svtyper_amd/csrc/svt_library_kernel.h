// svt_library_kernel.h -- the walk of svt_library_walk.h on the device (gfx950): inflated BAM bytes in HBM -> the library scans'
// tables in HBM.
//
// One wavefront (a workgroup of 64 lanes) per segment, as in svt_inflate_kernel.h: a round has hundreds to thousands of segments
// and that is where the parallelism is.  Lane 0 follows the segment's block_size chain 64 records at a time, the 64 lanes decode
// those records side by side (fixed fields, query length from the CIGAR, the tag walk up to RG, RG -> library), lane 0 applies
// what depends on file order (the running counts against the caps), the lanes add the accepted reads to the tables.
// X::sync() is __syncthreads(): in a one-wave workgroup it is the workgroup-scope fence between lane 0's LDS writes and the
// other lanes' reads.
//
// <false> counts (lw::SegCount per segment), the host turns the counts into caps, <true> accumulates: 64-bit integer atomics in
// HBM only (add, min, max) and a 32-bit counter for the overflow list -- no float atomics, no dependence on arrival order.
// LDS: lw::Scratch, 1 944 bytes per wave, static; 38 / 43 VGPRs, no scratch (profiles/library_scan_kernel_resources.txt).  Everything is written with ordinary vector stores from plain C++.
#ifndef SVT_LIBRARY_KERNEL_H
#define SVT_LIBRARY_KERNEL_H

#include "svt_library_walk.h"

namespace svt {

constexpr int kLibraryBlock = 64;

struct LibraryDevCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kLibraryBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ void add64(uint64_t* p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
    static __device__ __forceinline__ void min64(uint64_t* p, uint64_t v) { atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
    static __device__ __forceinline__ void max64(uint64_t* p, uint64_t v) { atomicMax(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
    static __device__ __forceinline__ uint32_t fetch_add32(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
};

template <bool kAccumulate>
__global__ __launch_bounds__(kLibraryBlock) void svt_library_kernel(const lw::Params P)
{
    __shared__ lw::Scratch S;
    const uint32_t si = blockIdx.x;
    if (si >= P.n_segments) return;
    lw::walk_segment<LibraryDevCtx, kAccumulate>(P, si, S);
}

}  // namespace svt

#endif  // SVT_LIBRARY_KERNEL_H

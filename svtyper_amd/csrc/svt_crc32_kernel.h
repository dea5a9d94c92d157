// svt_crc32_kernel.h -- svt_crc32.h on the device (gfx950): the CRC-32 of byte ranges in HBM, one wavefront per range.
//
// A workgroup is one wave of 64 lanes.  It stages crc::Tables (9.5 KiB: the eight byte tables and the powers of the tree) in LDS
// once and then takes the jobs blockIdx.x, blockIdx.x + gridDim.x, ...: the launch is sized to the device (a few waves per SIMD), not
// to the number of jobs, so the staging is paid once per wave and not once per member.  Every lane runs slicing-by-8 over its
// own chunk with 16-byte loads (the 64 lanes of a load touch 64 different 128-byte lines a chunk apart, each line is used up
// by its lane's next seven loads out of L1 / L2); the registers are joined through LDS (crc::Scratch), X::sync() is
// __syncthreads() -- in a one-wave workgroup the barrier costs nothing, what it brings is the LDS fence.
//
// The kernel runs behind svt_inflate_kernel on the same stream when the bytes are that kernel's: a kernel boundary orders its
// stores in front of these loads.  With `status` the job's CRC is compared with Job.expected: a member whose status is
// inf::INF_OK so far and whose CRC differs becomes inf::INF_CRC (a job that does not fit the bytes: inf::INF_MEMBER); a member
// that failed already is left alone and its bytes are not read.  With `crc_out` the CRCs are written.  Either may be null.
// Everything is written with ordinary vector stores from plain C++.
#ifndef SVT_CRC32_KERNEL_H
#define SVT_CRC32_KERNEL_H

#include "svt_crc32.h"
#include "svt_inflate.h"

namespace svt {

constexpr int kCrcBlock = 64;
constexpr uint32_t kCrcWavesPerCu = 16;     // workgroups of a launch per CU: four waves per SIMD, 16 x 9.75 KiB of the CU's 160 KiB of LDS

struct CrcDevCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kCrcBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(kCrcBlock) void svt_crc32_kernel(const uint8_t* __restrict__ bytes, uint64_t bytes_len, const crc::Job* __restrict__ jobs,
                                                              uint32_t n, const crc::Tables* __restrict__ tables, uint32_t* __restrict__ crc_out,
                                                              uint32_t* status)
{
    __shared__ crc::Tables T;
    __shared__ crc::Scratch S;
    static_assert(sizeof(crc::Tables) % sizeof(uint32_t) == 0, "staged word by word");
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tables);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&T);
        for (uint32_t i = threadIdx.x; i < sizeof(crc::Tables) / sizeof(uint32_t); i += kCrcBlock) dst[i] = src[i];
    }
    __syncthreads();
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {     // (every decision in here is the same for all lanes)
        const crc::Job j = jobs[k];
        if (status && status[k] != inf::INF_OK) {
            if (crc_out && threadIdx.x == 0) crc_out[k] = 0;
            continue;
        }
        const bool fits = j.len <= crc::kMaxLen && j.off <= bytes_len && j.len <= bytes_len - j.off;
        const uint32_t c = fits ? crc::crc_member<CrcDevCtx>(bytes + j.off, j.len, T, S) : 0;
        if (threadIdx.x == 0) {
            if (crc_out) crc_out[k] = c;
            if (status && (!fits || c != j.expected)) status[k] = fits ? (uint32_t)inf::INF_CRC : (uint32_t)inf::INF_MEMBER;
        }
    }
}

}  // namespace svt

#endif  // SVT_CRC32_KERNEL_H

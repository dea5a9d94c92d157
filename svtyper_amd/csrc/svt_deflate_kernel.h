// svt_deflate_kernel.h -- svt_deflate.h on the device (gfx950): payloads in HBM -> whole BGZF members side by side in HBM.
//
// One wavefront (a workgroup of 64 lanes) per member, the members blockIdx.x, blockIdx.x + gridDim.x, ...: the launch is sized to
// the device, as svt_crc32_kernel's is.  Lane l parses chunk l over its own hash table in LDS (dfl::Scratch<64>: 64 tables of
// 256 16-bit entries, entry e of lane l at table[e * 64 + l], 32 KiB, and 580 bytes for the bit counts and the bytes lanes
// share): four waves per CU by LDS.  X::sync() is __syncthreads() -- in a one-wave workgroup the barrier costs nothing, what it
// brings is the LDS fence between a lane's store of its count / head / tail and the other lanes' loads.
//
// A member's size is known only after its parse, so there are two kernels (the size and write pair of svt_dump_kernel.h):
//   svt_deflate_kernel       payload k -> the deflate bytes, into a slot of the worst-case size (dfl::slot_bytes: the payload
//                            and 31 bytes) behind where its header will go, and clen[k];
//   svt_deflate_pack_kernel  behind a prefix sum on the host: header, deflate bytes, CRC-32 and ISIZE of member k to out_off[k].
// The CRC-32s are svt_crc32_kernel's over the same jobs on the same stream.  Parsing twice across two launches instead would
// have cost the parse a third time (svt_deflate.h parses twice as it is) to save a copy of the compressed bytes, which are
// the smaller side.  Plain loads and stores and LDS integer operations only.  The fixed mode has no atomics of any kind; the
// dynamic mode (svt_deflate_kernel<dfl::kDynamic>, 37 816 bytes of LDS: still four waves per CU) adds its tokens' symbols into
// the member's histogram with atomicAdd on LDS counters -- integer sums, the same in any order -- and has no global atomics.
// svt_huffman_lengths_kernel runs dfl::code_lengths alone, one wavefront per histogram.
#ifndef SVT_DEFLATE_KERNEL_H
#define SVT_DEFLATE_KERNEL_H

#include "svt_crc32.h"
#include "svt_deflate.h"

namespace svt {

constexpr int kDeflateBlock = 64;
constexpr uint32_t kDeflateWavesPerCu = 4;  // 4 x 33 KiB of the CU's 160 KiB of LDS
constexpr int kDeflatePackBlock = 256;

struct DeflateDevCtx {
    static constexpr uint32_t kWidth = kDeflateBlock;
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kDeflateBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ void add(uint32_t* counter) { atomicAdd(counter, 1u); }     // (a counter in LDS)
};

// where member k's slot begins: the slots of the members in front (their payloads and 31 bytes each)
__host__ __device__ inline uint64_t deflate_slot_at(uint64_t payload_off, uint64_t k) { return payload_off + k * dfl::slot_bytes(0); }

// payload jobs[k] (crc::Job: off, len) of `bytes` -> slots + deflate_slot_at(off, k) + 18; clen[k]: its deflate bytes, 0: refused
template <uint32_t M>
__global__ __launch_bounds__(kDeflateBlock) void svt_deflate_kernel(const uint8_t* __restrict__ bytes, uint64_t bytes_len, const crc::Job* __restrict__ jobs,
                                                                    uint32_t n, uint8_t* __restrict__ slots, uint64_t slots_len, uint32_t* __restrict__ clen)
{
    __shared__ dfl::Scratch<kDeflateBlock, M> S;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {      // (every decision in here is the same for all lanes)
        const crc::Job j = jobs[k];
        const uint64_t at = deflate_slot_at(j.off, k);
        const bool fits = j.len <= dfl::kMaxPayload && j.off <= bytes_len && j.len <= bytes_len - j.off && at <= slots_len &&
                          dfl::slot_bytes(j.len) <= slots_len - at;
        const uint32_t c = fits ? dfl::deflate_member<DeflateDevCtx, M>(bytes + j.off, j.len, slots + at + dfl::kHeaderBytes, dfl::cdata_bound(j.len), S) : 0;
        if (threadIdx.x == 0) clen[k] = c;
    }
}

// histogram k (freq[k * symbols .. + symbols), symbols <= 286) -> its code lengths under `limit`, by dfl::code_lengths
__global__ __launch_bounds__(kDeflateBlock) void svt_huffman_lengths_kernel(const uint32_t* __restrict__ freq, uint32_t sets, uint32_t symbols, uint32_t limit,
                                                                            uint8_t* __restrict__ lengths)
{
    __shared__ uint32_t f[dfl::kLitSyms];
    __shared__ uint8_t len[dfl::kLitSyms];
    __shared__ dfl::Build B;
    if (symbols > dfl::kLitSyms || limit < 1 || limit > 15) return;
    for (uint32_t k = blockIdx.x; k < sets; k += gridDim.x) {
        __syncthreads();                                        // (nobody still reads len of the histogram before)
        for (uint32_t s = threadIdx.x; s < symbols; s += kDeflateBlock) f[s] = freq[(uint64_t)k * symbols + s];
        dfl::code_lengths<DeflateDevCtx>(f, symbols, limit, len, B);
        for (uint32_t s = threadIdx.x; s < symbols; s += kDeflateBlock) lengths[(uint64_t)k * symbols + s] = len[s];
    }
}

// member k: 18 header bytes, clen[k] deflate bytes out of its slot, crc[k], jobs[k].len -> out + out_off[k]
__global__ __launch_bounds__(kDeflatePackBlock) void svt_deflate_pack_kernel(const uint8_t* __restrict__ slots, uint64_t slots_len,
                                                                             const crc::Job* __restrict__ jobs, const uint32_t* __restrict__ clen,
                                                                             const uint32_t* __restrict__ crc, const uint64_t* __restrict__ out_off, uint32_t n,
                                                                             uint8_t* __restrict__ out, uint64_t out_len)
{
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const crc::Job j = jobs[k];
        const uint32_t c = clen[k];
        const uint64_t from = deflate_slot_at(j.off, k) + dfl::kHeaderBytes, to = out_off[k];
        const uint64_t size = (uint64_t)dfl::kHeaderBytes + c + dfl::kTrailerBytes;
        if (c == 0 || c > dfl::cdata_bound(j.len) || from > slots_len || c > slots_len - from || to > out_len || size > out_len - to) continue;
        uint8_t* m = out + to;
        if (threadIdx.x < dfl::kHeaderBytes) m[threadIdx.x] = dfl::header_byte(threadIdx.x, c);
        else if (threadIdx.x < dfl::kHeaderBytes + dfl::kTrailerBytes)
            m[dfl::kHeaderBytes + c + (threadIdx.x - dfl::kHeaderBytes)] = dfl::trailer_byte(threadIdx.x - dfl::kHeaderBytes, crc[k], j.len);
        for (uint32_t i = threadIdx.x; i < c; i += kDeflatePackBlock) m[dfl::kHeaderBytes + i] = slots[from + i];
    }
}

}  // namespace svt

#endif  // SVT_DEFLATE_KERNEL_H

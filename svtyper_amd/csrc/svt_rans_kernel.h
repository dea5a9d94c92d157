// svt_rans_kernel.h -- svt_rans.h on the device (gfx950): rANS 4x8 blocks in HBM decoded by FOUR LANES EACH, one per state.
//
// A state's symbol search and advance need nothing of the other three; what the four share is the stream of renormalisation
// bytes, read in state order.  How many bytes a state takes (0, 1 or 2) follows from the state alone (rans::need), so every
// lane packs its need into one byte of a word, two xor-shuffles inside the quad give every lane all four, and each lane has its
// read offset and the stream's new position without a serial step.  The position is checked against the block's end before a
// byte behind it is read.
//
// A workgroup is one wave of 64 lanes; every decision in the loops is per quad, the shuffles are executed by all lanes.
//   * svt_rans_o0_kernel: sixteen order-0 blocks per wave, their cumulative tables (257 x u16 each) in 8 KiB of static LDS.
//     Lane 0 of a quad parses its block's table; the quad's lanes then take the symbols 4t + lane (round robin over one
//     output), the last 1 to 3 symbols come from the first states without an advance.
//   * svt_rans_o1_kernel: ONE order-1 block per wave: the tables of the contexts are 256 x 257 x u16 = 131 584 bytes of dynamic
//     LDS, which a CU holds once.  All 64 lanes zero them, lane 0 parses, lanes 0 .. 3 decode the four quarters of the output with
//     their own previous symbol as context, lane 3 the remainder.  Sixty lanes idle: this is the shape the four-lane design is
//     worst at, and tools/cram_ab.py measures it alone.
// Both kernels take the jobs blockIdx.x, blockIdx.x + gridDim.x, ...  A block that is refused gets its status and a zeroed output
// range, as on the host.  Byte loads and byte stores from plain C++; nothing but vector memory instructions.
#ifndef SVT_RANS_KERNEL_H
#define SVT_RANS_KERNEL_H

#include "svt_rans.h"

namespace svt {

constexpr int kRansBlock = 64;
constexpr uint32_t kRansQuads = kRansBlock / 4;
constexpr uint32_t kRansO1Lds = 256 * rans::kCtx * sizeof(uint16_t);

// all four needs of the quad in one word, byte q being lane q's
__device__ __forceinline__ uint32_t rans_quad_needs(uint32_t mine, uint32_t q)
{
    uint32_t v = mine << (8 * q);
    v |= (uint32_t)__shfl_xor((int)v, 1);
    v |= (uint32_t)__shfl_xor((int)v, 2);
    return v;
}

// true in every lane of the quad when `flag` is in one of them
__device__ __forceinline__ bool rans_quad_any(bool flag)
{
    uint32_t v = flag;
    v |= (uint32_t)__shfl_xor((int)v, 1);
    v |= (uint32_t)__shfl_xor((int)v, 2);
    return v != 0;
}

// The steps of a quad: `steps` symbols per lane from the states behind the table at in[at].  Lane q writes out[first + t * stride];
// order 1 looks its table up by its previous symbol.  Runs in all lanes of the wave (`live`: the quad has a block and is not
// refused yet); a quad that is refused leaves with its status, the others go on.  The stream's position comes back in `at`.
template <bool ORDER1>
__device__ __forceinline__ uint32_t rans_quad_steps(bool live, const uint16_t* C, const uint8_t* in, uint32_t in_len, uint32_t& at, uint32_t& R,
                                                    uint32_t& ctx, uint8_t* out, uint32_t first, uint32_t stride, uint32_t steps, uint32_t q)
{
    uint32_t status = rans::RANS_OK;
    uint32_t t = 0;
    while (__any(live && t < steps)) {
        const bool on = live && t < steps;
        rans::Step st{0, 0, false};
        if (on) st = rans::advance(ORDER1 ? C + ctx * rans::kCtx : C, R);
        const bool bad = rans_quad_any(on && st.bad);
        const uint32_t n = on ? rans::need(st.x) : 0u;
        const uint32_t needs = rans_quad_needs(n, q);
        const uint32_t before = (needs & ((1u << (8 * q)) - 1u)) * 0x01010101u >> 24;      // (the sum of the bytes below mine)
        const uint32_t total = needs * 0x01010101u >> 24;
        if (on) {
            if (bad) {
                status = rans::RANS_SYMBOL;
                live = false;
            } else if (total > in_len - at) {
                status = rans::RANS_INPUT;
                live = false;
            } else {
                R = rans::refill(st.x, in + at + before, n);
                at += total;
                out[first + t * stride] = (uint8_t)st.sym;
                ctx = st.sym;
            }
        }
        ++t;
    }
    return status;
}

__global__ __launch_bounds__(kRansBlock) void svt_rans_o0_kernel(const uint8_t* __restrict__ data, uint8_t* __restrict__ out_base,
                                                                 const rans::Job* __restrict__ jobs, uint32_t n, uint32_t* __restrict__ status)
{
    __shared__ uint16_t T[kRansQuads][rans::kCtx + 1];
    const uint32_t quad = threadIdx.x >> 2, q = threadIdx.x & 3;
    for (uint64_t base = (uint64_t)blockIdx.x * kRansQuads; base < n; base += (uint64_t)gridDim.x * kRansQuads) {
        const uint64_t k = base + quad;
        bool live = k < n;
        rans::Job j{0, 0, 0, 0, 0, 0};
        if (live) j = jobs[k];
        const uint8_t* in = data + j.in_off;
        uint8_t* out = out_base + j.out_off;
        uint16_t* C = T[quad];
        __syncthreads();                                                  // (the round before has left the tables)
        for (uint32_t i = q; i < rans::kCtx; i += 4) C[i] = 0;
        __syncthreads();
        uint32_t st = rans::RANS_OK, at = 0;
        if (live && j.out_len && q == 0) {
            rans::In r{in, 0, j.in_len, false};
            if (!rans::parse_context(r, C)) st = rans::RANS_FREQ;
            else if (j.in_len - r.at < 16) st = rans::RANS_INPUT;
            at = r.at;
        }
        __syncthreads();
        st = (uint32_t)__shfl((int)st, (int)(threadIdx.x & ~3u));
        at = (uint32_t)__shfl((int)at, (int)(threadIdx.x & ~3u));
        const bool work = live && j.out_len && st == rans::RANS_OK;
        uint32_t R = 0, ctx = 0;
        if (work) R = rans::le32(in + at + 4 * q);
        at += 16;
        const uint32_t steps = j.out_len >> 2;
        const uint32_t s2 = rans_quad_steps<false>(work, C, in, j.in_len, at, R, ctx, out, q, 4, steps, q);
        bool tail_bad = false;
        if (work && s2 == rans::RANS_OK && q < (j.out_len & 3)) {
            const rans::Step s = rans::advance(C, R);
            tail_bad = s.bad;
            if (!s.bad) out[4 * steps + q] = (uint8_t)s.sym;
        }
        tail_bad = rans_quad_any(tail_bad);
        if (st == rans::RANS_OK) st = s2 ? s2 : tail_bad ? (uint32_t)rans::RANS_SYMBOL : (uint32_t)rans::RANS_OK;
        if (live) {
            if (st != rans::RANS_OK)
                for (uint32_t i = q; i < j.out_len; i += 4) out[i] = 0;
            if (q == 0) status[j.block] = st;
        }
    }
}

__global__ __launch_bounds__(kRansBlock) void svt_rans_o1_kernel(const uint8_t* __restrict__ data, uint8_t* __restrict__ out_base,
                                                                 const rans::Job* __restrict__ jobs, uint32_t n, uint32_t* __restrict__ status)
{
    extern __shared__ uint16_t rans_o1_tables[];                          // [256][257]
    uint16_t* C = rans_o1_tables;
    const uint32_t lane = threadIdx.x, q = lane & 3;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {                // (every decision on k is the wave's)
        const rans::Job j = jobs[k];
        const uint8_t* in = data + j.in_off;
        uint8_t* out = out_base + j.out_off;
        __syncthreads();
        {
            uint32_t* w = reinterpret_cast<uint32_t*>(C);
            for (uint32_t i = lane; i < kRansO1Lds / 4; i += kRansBlock) w[i] = 0;
        }
        __syncthreads();
        uint32_t st = rans::RANS_OK, at = 0;
        if (lane == 0) {
            rans::In r{in, 0, j.in_len, false};
            if (!rans::parse_order1(r, C)) st = rans::RANS_FREQ;
            else if (j.in_len - r.at < 16) st = rans::RANS_INPUT;
            at = r.at;
        }
        __syncthreads();
        st = (uint32_t)__shfl((int)st, 0);
        at = (uint32_t)__shfl((int)at, 0);
        const bool work = lane < 4 && st == rans::RANS_OK;
        uint32_t R = 0, ctx = 0;
        if (work) R = rans::le32(in + at + 4 * q);
        at += 16;
        const uint32_t steps = j.out_len >> 2;
        uint32_t s2 = rans_quad_steps<true>(work, C, in, j.in_len, at, R, ctx, out, q * steps, 1, steps, q);
        if (work && s2 == rans::RANS_OK && lane == 3) {                  // the last quarter takes the remainder
            for (uint32_t i = 4 * steps; i < j.out_len; ++i) {
                const rans::Step s = rans::advance(C + ctx * rans::kCtx, R);
                if (s.bad) { s2 = rans::RANS_SYMBOL; break; }
                const uint32_t nb = rans::need(s.x);
                if (nb > j.in_len - at) { s2 = rans::RANS_INPUT; break; }
                R = rans::refill(s.x, in + at, nb);
                at += nb;
                out[i] = (uint8_t)s.sym;
                ctx = s.sym;
            }
        }
        // lanes 0 .. 3 hold the quad's status of the steps; lane 3 also that of the remainder
        const uint32_t s_steps = (uint32_t)__shfl((int)s2, 0), s_rest = (uint32_t)__shfl((int)s2, 3);
        if (st == rans::RANS_OK) st = s_steps ? s_steps : s_rest;
        if (st != rans::RANS_OK)
            for (uint32_t i = lane; i < j.out_len; i += kRansBlock) out[i] = 0;
        if (lane == 0) status[j.block] = st;
    }
}

}  // namespace svt

#endif  // SVT_RANS_KERNEL_H

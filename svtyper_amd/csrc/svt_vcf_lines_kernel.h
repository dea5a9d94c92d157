// svt_vcf_lines_kernel.h -- svt_vcf_lines.h on the device (gfx950): VCF text in HBM -> its line table in text order, and the
// gather that writes the lines in another order into a second buffer.
//
// A tile is tbx::kTile = 4096 bytes of text and belongs to one wavefront: four rounds of 64 lanes x 16 bytes, one 16-byte load
// per lane (the text begins on an allocation's boundary, so every load but the text's last is whole and aligned; the tail is
// read byte by byte).  A lane's newlines are a 16-bit mask made from its four words with integer operations.
//   svt_vcf_count_kernel    popcount of the masks, summed over the wave by shuffles: counts[tile]
//   (the host)              an exclusive prefix sum of counts, as the evidence kernels' offsets are made: base[tile]
//   svt_vcf_starts_kernel   the same masks again; newline g of the text ends line g, so line g + 1 begins behind it: a lane
//                           ranks its newlines by a shuffle scan behind base[tile] and stores lines[g + 1].off
//   svt_vcf_parse_kernel    one lane per line: its length is the next line's start less its own (known only now, which is why
//                           this is a launch of its own), then tbx::parse_line over its first eight columns
// The table is in text order by construction: where a record goes is the rank of its newline, nothing is claimed with an
// atomic, and no kernel here has one.
//   svt_vcf_gather_kernel   output lines 64 w .. 64 w + 63 belong to wavefront w: lane l copies line 64 w + l itself where it is
//                           short (at most kGatherShort bytes), then the wave copies the longer ones together, lane l bytes
//                           l, l + 64, ...  Where a line goes is a prefix sum of the lengths in the new order, made on the
//                           host; the host twin is a loop of memcpy (tbx::gather_host).
// Every load is checked against the text's length, every store against the table's or the output's.
#ifndef SVT_VCF_LINES_KERNEL_H
#define SVT_VCF_LINES_KERNEL_H

#include "svt_vcf_lines.h"

namespace svt {

constexpr int kLinesBlock = 256;                    // four wavefronts, a tile each
constexpr uint32_t kLinesWaves = kLinesBlock / 64;
constexpr uint32_t kGatherShort = 32;

// bit j: byte j of the word is '\n' (exact: no carry runs from one byte into the next)
__device__ __forceinline__ uint32_t newline_bits(uint32_t x)
{
    const uint32_t y = x ^ 0x0A0A0A0Au;
    const uint32_t t = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);     // 0x80 where the byte of y is 0
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

// bit j: text[at + j] is '\n', for the 16 bytes at `at` (a multiple of 16) that lie inside the text
__device__ __forceinline__ uint32_t newline_mask16(const uint8_t* __restrict__ text, uint64_t len, uint64_t at)
{
    if (at >= len) return 0;
    if (len - at >= 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + at);
        return newline_bits(v.x) | newline_bits(v.y) << 4 | newline_bits(v.z) << 8 | newline_bits(v.w) << 12;
    }
    uint32_t m = 0;
    for (uint32_t j = 0; at + j < len; ++j) m |= (uint32_t)(text[at + j] == '\n') << j;
    return m;
}

__global__ __launch_bounds__(kLinesBlock) void svt_vcf_count_kernel(const uint8_t* __restrict__ text, uint64_t len, uint64_t n_tiles,
                                                                    uint32_t* __restrict__ counts)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t t = (uint64_t)blockIdx.x * kLinesWaves + wave; t < n_tiles; t += (uint64_t)gridDim.x * kLinesWaves) {
        uint32_t c = 0;
        for (uint32_t r = 0; r < 4; ++r) c += __popc(newline_mask16(text, len, t * tbx::kTile + r * 1024 + lane * 16));
        for (int d = 32; d; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0) counts[t] = c;
    }
}

// lines[g + 1].off for every newline g of the text that a line follows; lines[0].off = 0
__global__ __launch_bounds__(kLinesBlock) void svt_vcf_starts_kernel(const uint8_t* __restrict__ text, uint64_t len, uint64_t n_tiles,
                                                                     const uint64_t* __restrict__ base, svt_tbx_line* __restrict__ lines, uint64_t n_lines)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_lines) lines[0].off = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kLinesWaves + wave; t < n_tiles; t += (uint64_t)gridDim.x * kLinesWaves) {
        uint64_t running = base[t];
        for (uint32_t r = 0; r < 4; ++r) {          // (every lane takes every round: the shuffles are the whole wave's)
            const uint64_t at = t * tbx::kTile + r * 1024 + lane * 16;
            uint32_t m = newline_mask16(text, len, at);
            const uint32_t c = __popc(m);
            uint32_t inc = c;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d);
                if ((int)lane >= d) inc += v;
            }
            uint64_t g = running + inc - c;
            running += __shfl(inc, 63);
            while (m) {
                const uint64_t next = at + (uint32_t)(__ffs(m) - 1) + 1;
                m &= m - 1;
                if (next < len && g + 1 < n_lines) lines[g + 1].off = next;
                ++g;
            }
        }
    }
}

__global__ __launch_bounds__(kLinesBlock) void svt_vcf_parse_kernel(const uint8_t* __restrict__ text, uint64_t len, svt_tbx_line* __restrict__ lines,
                                                                    uint64_t n_lines)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kLinesBlock + threadIdx.x; i < n_lines; i += (uint64_t)gridDim.x * kLinesBlock) {
        svt_tbx_line r;
        r.off = lines[i].off;
        const uint64_t end = i + 1 < n_lines ? lines[i + 1].off : len;
        if (r.off <= end && end <= len) {
            r.len = end - r.off;
            tbx::parse_line(text + r.off, r.len, r);
        } else {                                    // (starts that do not rise: not this launch's table)
            r.len = 0;
            r.beg = r.end = r.chrom_len = 0;
            r.flags = SVT_TBX_BAD;
        }
        lines[i].len = r.len;
        lines[i].beg = r.beg;
        lines[i].end = r.end;
        lines[i].chrom_len = r.chrom_len;
        lines[i].flags = r.flags;
    }
}

// line lines[perm[j]] of text -> out + dst_off[j], j < n_perm.  Row: a table's record with `off` and `len` (svt_tbx_line; svt_bam_span,
// whose "lines" are the records of svt_bam_sort_kernel.h)
template <typename Row>
__global__ __launch_bounds__(kLinesBlock) void svt_vcf_gather_kernel(const uint8_t* __restrict__ text, uint64_t len, const Row* __restrict__ lines,
                                                                     uint64_t n, const uint64_t* __restrict__ perm, const uint64_t* __restrict__ dst_off,
                                                                     uint64_t n_perm, uint8_t* __restrict__ out, uint64_t out_len)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t groups = (n_perm + 63) / 64;
    for (uint64_t w = (uint64_t)blockIdx.x * kLinesWaves + wave; w < groups; w += (uint64_t)gridDim.x * kLinesWaves) {
        const uint64_t j = w * 64 + lane;
        unsigned long long src = 0, dst = 0, size = 0;
        if (j < n_perm && perm[j] < n) {
            const uint64_t l_off = lines[perm[j]].off, l_len = lines[perm[j]].len;
            const uint64_t d = dst_off[j];
            if (l_off <= len && l_len <= len - l_off && d <= out_len && l_len <= out_len - d) {
                src = l_off;
                dst = d;
                size = l_len;
            }
        }
        if (size <= kGatherShort)
            for (uint32_t i = 0; i < (uint32_t)size; ++i) out[dst + i] = text[src + i];
        const uint32_t held = (uint32_t)(n_perm - w * 64 < 64 ? n_perm - w * 64 : 64);
        for (uint32_t k = 0; k < held; ++k) {       // (the same lines for every lane: no lane leaves the shuffles)
            const unsigned long long size_k = __shfl(size, (int)k);
            if (size_k <= kGatherShort) continue;
            const unsigned long long src_k = __shfl(src, (int)k), dst_k = __shfl(dst, (int)k);
            for (unsigned long long i = lane; i < size_k; i += 64) out[dst_k + i] = text[src_k + i];
        }
    }
}

}  // namespace svt

#endif  // SVT_VCF_LINES_KERNEL_H

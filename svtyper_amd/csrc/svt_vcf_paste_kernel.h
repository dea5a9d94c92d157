// svt_vcf_paste_kernel.h -- svt_vcf_paste.h on the device (gfx950): the lines of a master and of N inputs in HBM under one line
// table -> the joined lines.  The data shape is "a line is wide, lanes go over inputs": ONE WAVEFRONT PER OUTPUT LINE.
//
//   svt_paste_measure_kernel   input s of line j is lane s % 64's, in strides of 64 inputs.  A lane runs paste::measure_input on its
//                              input's line (every lane runs paste::measure_master on the master's: the same addresses, one
//                              fetch for the wave).  Across the lanes, by shuffles and without an atomic: the allele and
//                              non-reference counts (summed), the marks (or-ed), the --safe verdict (the lowest offending input:
//                              a minimum), and the exclusive prefix of the parts' lengths with a tab each, carried from stride to
//                              stride; a lane stores where its part lies and goes (paste::Place, 12 bytes per line and input).
//                              The QUALs are NOT tree-reduced: every lane reads the stride's values lane by lane (a shuffle with a
//                              uniform index) and adds them in file order behind the master's, so the sum is the one a loop over
//                              the files gives, bit for bit.  One svt_paste_line per line.
//   (the host)                 plan_block: the marked lines by slow_line, the other lines' first columns (snprintf is the exact
//                              formatter: the device hands over a double and counts, never text), the sizes summed.
//   svt_paste_write_kernel<G>  the line's first columns with lanes over bytes, then the parts: G lanes share one part, 64 / G
//                              parts are copied at a time (G = 1: a lane per part; 16: a quarter of the wave; 64: the wave).
//                              Marked lines are skipped: the host writes them into the same buffer.
// Every load is checked against its line's length, which is checked against the text's; every store against the line's
// measured size, which is checked against the output's.  No LDS, no scratch memory, no inline assembly.
#ifndef SVT_VCF_PASTE_KERNEL_H
#define SVT_VCF_PASTE_KERNEL_H

#include "svt_vcf_paste.h"

namespace svt {

constexpr int kPasteBlock = 256;                    // four wavefronts, a line each
constexpr uint32_t kPasteWaves = kPasteBlock / 64;

// line i of the table inside the text: its bytes, or false
__device__ __forceinline__ bool paste_line_at(const svt_tbx_line* __restrict__ lines, uint64_t n_table, uint64_t len, uint64_t i, uint64_t& off, uint64_t& size)
{
    off = size = 0;
    if (i >= n_table) return false;
    off = lines[i].off;
    size = lines[i].len;
    if (off <= len && size <= len - off) return true;
    off = size = 0;
    return false;
}

__device__ __forceinline__ uint32_t paste_wave_sum(uint32_t v)
{
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(kPasteBlock) void svt_paste_measure_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                        uint64_t n_table, const uint64_t* __restrict__ first_line, uint32_t n_inputs,
                                                                        uint64_t n_lines, uint32_t flags, svt_paste_line* __restrict__ results,
                                                                        paste::Place* __restrict__ places)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t j = (uint64_t)blockIdx.x * kPasteWaves + wave; j < n_lines; j += (uint64_t)gridDim.x * kPasteWaves) {
        uint64_t m_off, m_len;
        const bool m_ok = paste_line_at(lines, n_table, len, first_line[0] + j, m_off, m_len);
        paste::Master m;
        paste::measure_master(text + m_off, m_len, flags, m);
        uint32_t slow = m_ok ? m.slow : SVT_PASTE_SLOW_COLUMNS;
        double qual = m.qual;                       // (the same in every lane)
        uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0, nonref = 0;
        uint32_t unsafe = 0xFFFFFFFFu;              // 4 * input + field of this lane's lowest offending input
        uint32_t part_total = 0;
        for (uint32_t base = 0; base < n_inputs; base += 64) {      // (every lane takes every stride: the shuffles are the whole wave's)
            const uint32_t s = base + lane;
            paste::Input in;
            in.qual = 0.0;
            in.lo = in.hi = 0;
            in.nonref = in.slow = in.part_b = in.part_len = 0;
            in.unequal = paste::kNoField;
            if (s < n_inputs) {
                uint64_t off, size;
                if (paste_line_at(lines, n_table, len, first_line[s + 1] + j, off, size)) paste::measure_input(text + off, size, text + m_off, m, flags, in);
                else in.slow = SVT_PASTE_SLOW_COLUMNS;
            }
            slow |= in.slow;
            c0 += (uint32_t)in.lo & 0xFFFFu;
            c1 += (uint32_t)(in.lo >> 16) & 0xFFFFu;
            c2 += (uint32_t)(in.lo >> 32) & 0xFFFFu;
            c3 += (uint32_t)(in.lo >> 48);
            c4 += (uint32_t)in.hi & 0xFFFFu;
            c5 += (uint32_t)(in.hi >> 16) & 0xFFFFu;
            c6 += (uint32_t)(in.hi >> 32) & 0xFFFFu;
            c7 += (uint32_t)(in.hi >> 48);
            nonref += in.nonref;
            if (in.unequal != paste::kNoField && unsafe == 0xFFFFFFFFu) unsafe = 4 * s + in.unequal;
            // where the part goes: behind the parts of the inputs in front of it, each with its tab
            const uint32_t width = in.part_len ? in.part_len + 1 : 0;
            uint32_t inc = width;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d);
                if ((int)lane >= d) inc += v;
            }
            if (s < n_inputs) places[j * n_inputs + s] = paste::Place{in.part_b, in.part_len, part_total + inc - width};
            part_total += __shfl(inc, 63);
            // the QUALs in file order: every lane adds the same values in the same order
            const uint32_t held = n_inputs - base < 64 ? n_inputs - base : 64;
            for (uint32_t k = 0; k < held; ++k) qual += __shfl(in.qual, (int)k);
        }
        for (int d = 32; d; d >>= 1) {
            slow |= __shfl_xor(slow, d);
            const uint32_t other = __shfl_xor(unsafe, d);
            unsafe = other < unsafe ? other : unsafe;
        }
        c0 = paste_wave_sum(c0);
        c1 = paste_wave_sum(c1);
        c2 = paste_wave_sum(c2);
        c3 = paste_wave_sum(c3);
        c4 = paste_wave_sum(c4);
        c5 = paste_wave_sum(c5);
        c6 = paste_wave_sum(c6);
        c7 = paste_wave_sum(c7);
        nonref = paste_wave_sum(nonref);
        if (lane == 0) {
            svt_paste_line r;
            r.qual = qual;
            r.counts[0] = c0;
            r.counts[1] = c1;
            r.counts[2] = c2;
            r.counts[3] = c3;
            r.counts[4] = c4;
            r.counts[5] = c5;
            r.counts[6] = c6;
            r.counts[7] = c7;
            r.nonref = nonref;
            r.flags = slow | (unsafe != 0xFFFFFFFFu ? SVT_PASTE_UNSAFE : 0u);
            r.bad_input = unsafe != 0xFFFFFFFFu ? unsafe >> 2 : paste::kNoInput;
            r.bad_field = unsafe != 0xFFFFFFFFu ? unsafe & 3u : paste::kNoField;
            r.part_len = part_total;
            r.line_len = 0;
            results[j] = r;
        }
    }
}

// prefix_off / out_off [0 .. n_lines]: where the lines' first columns lie in prefixes[0, prefix_len) and the lines go in out[0, out_len)
template <int G>
__global__ __launch_bounds__(kPasteBlock) void svt_paste_write_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                      uint64_t n_table, const uint64_t* __restrict__ first_line, uint32_t n_inputs,
                                                                      uint64_t n_lines, const svt_paste_line* __restrict__ results,
                                                                      const paste::Place* __restrict__ places, const uint8_t* __restrict__ prefixes,
                                                                      uint64_t prefix_len, const uint64_t* __restrict__ prefix_off,
                                                                      const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out, uint64_t out_len)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t j = (uint64_t)blockIdx.x * kPasteWaves + wave; j < n_lines; j += (uint64_t)gridDim.x * kPasteWaves) {
        if (results[j].flags & paste::kSlowMask) continue;
        const uint64_t at = out_off[j], next = out_off[j + 1], pre_b = prefix_off[j], pre_e = prefix_off[j + 1];
        if (at > next || next > out_len || pre_b > pre_e || pre_e > prefix_len) continue;
        const uint64_t size = next - at, pre = pre_e - pre_b;
        if (size != pre + results[j].part_len + 1) continue;        // (not this launch's plan)
        uint8_t* line = out + at;
        for (uint64_t i = lane; i < pre; i += 64) line[i] = prefixes[pre_b + i];
        for (uint32_t s = lane / G; s < n_inputs; s += 64 / G) {
            const paste::Place pl = places[j * n_inputs + s];
            if (!pl.len) continue;
            uint64_t off, src_len;
            if (!paste_line_at(lines, n_table, len, first_line[s + 1] + j, off, src_len)) continue;
            if (pl.src > src_len || pl.len > src_len - pl.src) continue;
            const uint8_t* src = text + off + pl.src;
            for (uint32_t i = lane % G; i <= pl.len; i += G) {
                const uint64_t d = pre + pl.dst + i;
                if (d < size) line[d] = i ? src[i - 1] : (uint8_t)'\t';
            }
        }
        if (lane == 0) line[size - 1] = '\n';
    }
}

}  // namespace svt

#endif  // SVT_VCF_PASTE_KERNEL_H

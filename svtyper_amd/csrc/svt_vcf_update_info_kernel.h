// svt_vcf_update_info_kernel.h -- svt_vcf_update_info.h on the device (gfx950): the body lines of a cohort VCF in HBM under their
// line table -> one svt_update_info_line per line.  The data shape is paste's and classify's, "a line is wide, lanes go over
// samples": ONE WORKGROUP OF 256 LANES PER LINE, every line does work.  Part of svt_small_kernels.hip, launched through
// update_info_launch.
//
//   head      once per line: wavefront 0 finds the first nine tabs, 64 bytes a step (a ballot, a lane stores the tab it holds into
//             LDS); lane 0 runs update_info::check_head on POS, QUAL and FORMAT (INFO, the long column, is only passed over) and
//             the result is broadcast through LDS
//   starts    the bytes behind the ninth tab in 16-byte pieces, aligned in memory, a lane each and 256 side by side: one 128-bit
//             load where the piece lies inside the text (bytes in front of the column and behind the line are masked away), the
//             tabs as a 16-bit mask, an exclusive scan over the workgroup (shuffles inside a wavefront, the four totals through
//             LDS, the count carried from step to step), and every lane writes where the columns behind its tabs begin into LDS.
//             One pass.  Not one column per sample of the header: the line is marked
//   samples   sample s is lane s % 256's, in strides of 256: update_info::parse_sample, ONCE per column; AP, AS, the positives and
//             the marks meet by shuffles and one exchange through LDS; the SQ of a positive sample, +0.0 for any other, is staged
//             in LDS at the sample's index
//   sum_sq    NOT tree-reduced: one lane adds the staged values in sample order from +0.0, eight loads ahead of eight dependent
//             adds, so the sum is the host loop's, bit for bit (the file is compiled with -ffp-contract=off and without fast-math)
// 49 KB of LDS per workgroup, three workgroups to a CU.  Every load is checked against its line's length, which is checked against
// the text's; every LDS index against the capacity.  No scratch memory, no atomics, no inline assembly.
#ifndef SVT_VCF_UPDATE_INFO_KERNEL_H
#define SVT_VCF_UPDATE_INFO_KERNEL_H

#include "svt_vcf_update_info.h"

namespace svt {

constexpr int kUpdateInfoBlock = (int)update_info::kBlock;

struct UpdateInfoShared {
    double sq[update_info::kCapacity];
    uint32_t starts[update_info::kCapacity + 1];   // starts[n]: behind the line's end, as if a tab stood there
    update_info::Head head;
    uint32_t tab[9], n_tabs;
    uint32_t scan[2][4];
    unsigned long long wave_pe[4], wave_sr[4];
    uint32_t wave_pos[4], wave_slow[4];
};

// bit k: byte k of the word is a tab
__device__ __forceinline__ uint32_t update_info_tabs(uint32_t word)
{
    const uint32_t t = word ^ 0x09090909u, nonzero = ((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t, z = ~nonzero & 0x80808080u;
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

__global__ __launch_bounds__(kUpdateInfoBlock) void svt_update_info_kernel(const uint8_t* __restrict__ text, uint64_t len,
                                                                         const svt_tbx_line* __restrict__ lines, uint64_t n_lines,
                                                                         const uint8_t* __restrict__ format_table, update_info::Params pr,
                                                                         svt_update_info_line* __restrict__ results)
{
    using namespace update_info;
    __shared__ UpdateInfoShared sh;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = pr.n_samples;
    for (uint64_t j = blockIdx.x; j < n_lines; j += gridDim.x) {
        __syncthreads();                            // (the line before is done with the LDS)
        uint64_t off = lines[j].off, size = lines[j].len;
        if (off > len || size > len - off) off = size = 0;
        const uint8_t* p = text + off;
        const uint32_t n_line = stripped_length(p, size);
        // the head, once
        if (wave == 0) {
            uint32_t found = 0;
            for (uint32_t base = 0; base < n_line && found < 9; base += 64) {
                const uint32_t i = base + lane;
                const bool is_tab = i < n_line && p[i] == '\t';
                const unsigned long long mask = __ballot(is_tab);
                const uint32_t k = found + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
                if (is_tab && k < 9) sh.tab[k] = i;
                found += (uint32_t)__popcll(mask);
            }
            if (lane == 0) sh.n_tabs = found < 9 ? found : 9;
        }
        __syncthreads();
        if (tid == 0) {
            Tabs t;
            t.count = sh.n_tabs;
#pragma unroll
            for (uint32_t c = 0; c < 9; ++c) t.tab[c] = c < t.count ? sh.tab[c] : n_line;
            Head scanned;
            check_head(p, n_line, size > paste::kMaxLine, t, format_table, pr.format_len, scanned);
            sh.head = scanned;
        }
        __syncthreads();
        const Head h = sh.head;
        uint32_t slow = h.slow;
        if (!slow && (!n || n > kCapacity)) slow = SVT_UPDATE_INFO_SLOW_CAPACITY;
        if (slow) {
            if (tid == 0) results[j] = marked_record(slow);
            continue;
        }
        // where the sample columns begin
        const uint32_t span = h.n - h.samples_b;
        const uintptr_t a_text = (uintptr_t)text, a_line = (uintptr_t)p, a_first = a_line + h.samples_b, a_0 = a_first & ~(uintptr_t)15;
        const uint32_t n_chunks = span ? (uint32_t)((a_first + span - a_0 + 15) >> 4) : 0;
        uint32_t carried = 0;
        for (uint32_t base = 0, step = 0; base < n_chunks; base += kUpdateInfoBlock, ++step) {
            const uint32_t c = base + tid;
            uint32_t m = 0;
            int64_t at_0 = 0;                       // where the piece's first byte lies in the line (the first piece: maybe in front of the column)
            if (c < n_chunks) {
                const uintptr_t a_c = a_0 + ((uintptr_t)c << 4);
                at_0 = (int64_t)a_c - (int64_t)a_line;
                const int64_t lo64 = (int64_t)h.samples_b - at_0, hi64 = (int64_t)h.n - at_0;
                const uint32_t lo = lo64 > 0 ? (uint32_t)lo64 : 0u, hi = hi64 < 16 ? (uint32_t)hi64 : 16u;
                if (a_c >= a_text && a_c + 16 <= a_text + len) {
                    const uint4 w = *reinterpret_cast<const uint4*>(a_c);
                    m = update_info_tabs(w.x) | update_info_tabs(w.y) << 4 | update_info_tabs(w.z) << 8 | update_info_tabs(w.w) << 12;
                } else {
                    for (uint32_t k = lo; k < hi; ++k) m |= (uint32_t)(p[at_0 + k] == '\t') << k;
                }
                m &= ((1u << hi) - 1u) & ~((1u << lo) - 1u);
            }
            const uint32_t count = (uint32_t)__popc(m);
            uint32_t inc = count;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d);
                if ((int)lane >= d) inc += v;
            }
            if (lane == 63) sh.scan[step & 1][wave] = inc;
            __syncthreads();                        // (the two rows in turn: a wavefront two steps ahead has passed the barrier between)
            uint32_t before = inc - count, total = 0;
            for (uint32_t w = 0; w < 4; ++w) {
                const uint32_t of_wave = sh.scan[step & 1][w];
                before += w < wave ? of_wave : 0u;
                total += of_wave;
            }
            for (uint32_t at = carried + before + 1; m; ++at) {
                const uint32_t k = (uint32_t)__ffs((int)m) - 1;
                m &= m - 1;
                if (at < n) sh.starts[at] = (uint32_t)(at_0 + k) + 1;
            }
            carried += total;
        }
        if ((span ? carried + 1 : 0u) != n) {
            if (tid == 0) results[j] = marked_record(SVT_UPDATE_INFO_SLOW_COLUMNS);
            continue;
        }
        if (tid == 0) {
            sh.starts[0] = h.samples_b;
            sh.starts[n] = h.n + 1;
        }
        __syncthreads();
        // the samples, each column once
        unsigned long long pe = 0, sr = 0;
        uint32_t num_pos = 0;
        for (uint32_t s = tid; s < n; s += kUpdateInfoBlock) {
            const uint32_t b = sh.starts[s], e = sh.starts[s + 1] - 1;
            if (b > e || e > h.n) {
                slow |= SVT_UPDATE_INFO_SLOW_SAMPLE;
                sh.sq[s] = 0.0;
                continue;
            }
            Sample sm;
            parse_sample(p, b, e, h, sm);
            slow |= sm.slow;
            pe += sm.ap;
            sr += sm.as;
            num_pos += sm.positive;
            sh.sq[s] = sm.sq;
        }
        for (int d = 32; d; d >>= 1) {
            pe += __shfl_xor(pe, d);
            sr += __shfl_xor(sr, d);
            num_pos += __shfl_xor(num_pos, d);
            slow |= __shfl_xor(slow, d);
        }
        if (lane == 0) {
            sh.wave_pe[wave] = pe;
            sh.wave_sr[wave] = sr;
            sh.wave_pos[wave] = num_pos;
            sh.wave_slow[wave] = slow;
        }
        __syncthreads();
        if (tid == 0) {
            slow = sh.wave_slow[0] | sh.wave_slow[1] | sh.wave_slow[2] | sh.wave_slow[3];
            svt_update_info_line r = marked_record(slow);
            if (!slow) {
                r.pe = (int64_t)(sh.wave_pe[0] + sh.wave_pe[1] + sh.wave_pe[2] + sh.wave_pe[3]);
                r.sr = (int64_t)(sh.wave_sr[0] + sh.wave_sr[1] + sh.wave_sr[2] + sh.wave_sr[3]);
                r.num_pos = sh.wave_pos[0] + sh.wave_pos[1] + sh.wave_pos[2] + sh.wave_pos[3];
                double sum = 0.0;                   // in sample order: the order is the contract
                uint32_t s = 0;
                for (; s + 8 <= n; s += 8) {
                    const double v0 = sh.sq[s], v1 = sh.sq[s + 1], v2 = sh.sq[s + 2], v3 = sh.sq[s + 3];
                    const double v4 = sh.sq[s + 4], v5 = sh.sq[s + 5], v6 = sh.sq[s + 6], v7 = sh.sq[s + 7];
                    sum += v0;
                    sum += v1;
                    sum += v2;
                    sum += v3;
                    sum += v4;
                    sum += v5;
                    sum += v6;
                    sum += v7;
                }
                for (; s < n; ++s) sum += sh.sq[s];
                r.sum_sq = bits_of(sum);
            }
            results[j] = r;
        }
    }
}

// the launch, for the entry point in the library's other translation unit (svt_entry_vcf_update_info.h)
void update_info_launch(unsigned grid, hipStream_t stream, const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n_lines,
                        const uint8_t* format_table, uint32_t n_samples, uint32_t format_len, svt_update_info_line* results)
{
    update_info::Params pr;
    pr.n_samples = n_samples;
    pr.format_len = format_len;
    hipLaunchKernelGGL(svt_update_info_kernel, dim3(grid), dim3(kUpdateInfoBlock), 0, stream, text, len, lines, n_lines, format_table, pr, results);
}

}  // namespace svt

#endif  // SVT_VCF_UPDATE_INFO_KERNEL_H

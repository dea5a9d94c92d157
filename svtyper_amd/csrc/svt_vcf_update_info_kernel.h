// svt_vcf_update_info_kernel.h -- svt_vcf_update_info.h on the device (gfx950): the body lines of a cohort VCF in HBM under their
// line table -> one svt_update_info_line per line.  The data shape is paste's and classify's, "a line is wide, lanes go over
// samples": ONE WORKGROUP OF 256 LANES PER LINE, every line does work.  Part of svt_small_kernels.hip, launched through
// update_info_launch.
//
//   head, starts   svt_vcf_cohort_line_kernel.h: the first nine columns once per line (update_info::check_head in one lane; INFO, the
//             long column, is only passed over), where the sample columns begin from 128-bit loads.  Not one column per sample of
//             the header: the line is marked
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
#include "svt_vcf_cohort_line_kernel.h"

namespace svt {

constexpr int kUpdateInfoBlock = kCohortBlock;

struct UpdateInfoShared {
    double sq[update_info::kCapacity];
    CohortLineShared<update_info::Head, update_info::kCapacity> line;
    unsigned long long wave_pe[4], wave_sr[4];
    uint32_t wave_pos[4], wave_slow[4];
};

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
        uint64_t size;
        const uint8_t* p = cohort_line(text, len, lines, j, size);
        const Head h = cohort_head(sh.line, p, size, [&](uint32_t n_line, bool too_long, const Tabs& t, Head& scanned) {
            check_head(p, n_line, too_long, t, format_table, pr.format_len, scanned);
        });
        uint32_t slow = h.slow;
        if (!slow && (!n || n > kCapacity)) slow = SVT_UPDATE_INFO_SLOW_CAPACITY;
        if (slow) {
            if (tid == 0) results[j] = marked_record(slow);
            continue;
        }
        if (cohort_starts(sh.line, text, len, p, h, n) != n) {
            if (tid == 0) results[j] = marked_record(SVT_UPDATE_INFO_SLOW_COLUMNS);
            continue;
        }
        // the samples, each column once
        unsigned long long pe = 0, sr = 0;
        uint32_t num_pos = 0;
        for (uint32_t s = tid; s < n; s += kUpdateInfoBlock) {
            const uint32_t b = sh.line.starts[s], e = sh.line.starts[s + 1] - 1;
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

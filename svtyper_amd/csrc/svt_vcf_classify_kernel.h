// svt_vcf_classify_kernel.h -- svt_vcf_classify.h on the device (gfx950): the body lines of a cohort VCF in HBM under their line
// table -> one svt_classify_line per line.  The data shape is paste's, "a line is wide, lanes go over samples", but a line's
// samples meet in an order statistic, so it is ONE WORKGROUP OF 256 LANES PER LINE (a line that is no DEL or DUP costs its
// first columns and nothing else).
//
//   head, starts   svt_vcf_cohort_line_kernel.h: the first nine columns once per line (classify::check_head in one lane), where the
//             sample columns begin from 128-bit loads.  Not one column per sample of the header: the line is marked
//   samples   sample s is lane s % 256's, in strides of 256: classify::parse_sample; the GT class in LDS; the marks or-ed and
//             the counts added by shuffles
//   low       the CN of the list the median is taken of as order-preserving keys in LDS (their places by an LDS counter: any
//             order, they are sorted next), padded to a power of two, a bitonic sort, the median; |cn - median| in place, the
//             sort again, the MAD; then the carriers against both (IEEE subtract, multiply by 2, compare), counted by shuffles
//   high      two passes of centred sums in double: a lane adds its samples in sample order, an xor butterfly joins a
//             wavefront's lanes, the four results meet as (w0 + w1) + (w2 + w3): the order classify::Tree restates
// A pass that needs a sample's numbers again parses the column again (its start is in LDS): 53 KB of LDS per workgroup, three
// workgroups to a CU.  Every load is checked against its line's length, which is checked against the text's; every LDS index
// against the capacity.  No scratch memory, no inline assembly.
#ifndef SVT_VCF_CLASSIFY_KERNEL_H
#define SVT_VCF_CLASSIFY_KERNEL_H

#include "svt_vcf_classify.h"
#include "svt_vcf_cohort_line_kernel.h"

namespace svt {

constexpr int kClassifyBlock = kCohortBlock;

struct ClassifyShared {
    uint64_t keys[classify::kCapacity];
    CohortLineShared<classify::Head, classify::kCapacity> line;
    uint8_t gt[classify::kCapacity];
    double wave_d[4];
    uint32_t wave_u[4];
    uint32_t counter;
};

// keys[0, m), m a power of two, ascending
__device__ __forceinline__ void classify_sort(uint64_t* keys, uint32_t m)
{
    for (uint32_t k = 2; k <= m; k <<= 1)
        for (uint32_t j = k >> 1; j; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < m; i += kClassifyBlock) {
                const uint32_t o = i ^ j;
                if (o > i && o < classify::kCapacity) {
                    const uint64_t a = keys[i], b = keys[o];
                    if ((a > b) == ((i & k) == 0)) {
                        keys[i] = b;
                        keys[o] = a;
                    }
                }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(kClassifyBlock) void svt_classify_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                      uint64_t n_lines, const uint8_t* __restrict__ male, const uint8_t* __restrict__ female,
                                                                      const uint8_t* __restrict__ excluded, const uint8_t* __restrict__ format_table,
                                                                      classify::Params pr, svt_classify_line* __restrict__ results)
{
    using namespace classify;
    __shared__ ClassifyShared sh;
    const uint32_t tid = threadIdx.x, n = pr.n_samples;
    for (uint64_t j = blockIdx.x; j < n_lines; j += gridDim.x) {
        __syncthreads();                            // (the line before is done with the LDS)
        uint64_t size;
        const uint8_t* p = cohort_line(text, len, lines, j, size);
        const Head h = cohort_head(sh.line, p, size, [&](uint32_t n_line, bool too_long, const Tabs& t, Head& scanned) {
            check_head(p, n_line, too_long, t, format_table, pr.format_len, scanned);
        });
        if (!h.svtype) {
            if (tid == 0) results[j] = empty_record(SVT_CLASSIFY_VERBATIM, 0);
            continue;
        }
        const uint32_t type = h.svtype == 1 ? SVT_CLASSIFY_DEL : 0u;
        uint32_t slow = h.slow;
        if (!slow && (!n || n > kCapacity)) slow = SVT_CLASSIFY_SLOW_CAPACITY;
        if (slow) {
            if (tid == 0) results[j] = empty_record(SVT_CLASSIFY_LOW, slow | type);
            continue;
        }
        if (cohort_starts(sh.line, text, len, p, h, n) != n) {
            if (tid == 0) results[j] = empty_record(SVT_CLASSIFY_LOW, SVT_CLASSIFY_SLOW_COLUMNS | type);
            continue;
        }
        const uint32_t* starts = sh.line.starts;
        // the samples: marks, GT classes, counts
        uint32_t n_pos = 0, male_alt = 0, female_alt = 0;
        for (uint32_t s = tid; s < n; s += kClassifyBlock) {
            const uint32_t b = starts[s], e = starts[s + 1] - 1;
            Sample sm;
            if (b > e || e > h.n) {
                slow |= SVT_CLASSIFY_SLOW_SAMPLE;
                sh.gt[s] = kGtOther;
                continue;
            }
            parse_sample(p, b, e, h, sm);
            slow |= sm.slow;
            sh.gt[s] = (uint8_t)sm.gt;
            if (h.sex && male[s] == SVT_CLASSIFY_NO_GENDER) slow |= SVT_CLASSIFY_SLOW_GENDER;
            if (excluded[s]) continue;
            n_pos += sm.gt != kGtMissing && sm.gt != kGtRef;
            const bool alt = sm.gt == kGtHet || sm.gt == kGtHom;
            male_alt += alt && male[s] == 1;
            female_alt += alt && female[s] == 1;
        }
        n_pos = block_sum(n_pos, sh.wave_u);
        slow = block_or(slow, sh.wave_u);
        svt_classify_line r = empty_record(n_pos < kMinPosForRegression ? SVT_CLASSIFY_LOW : SVT_CLASSIFY_HIGH, type);
        r.n_pos = n_pos;
        slow |= route_keys(r.route, h);
        if (slow) {
            r.flags |= slow;
            if (tid == 0) results[j] = r;
            continue;
        }
        const bool del = h.svtype == 1;
        if (r.route == SVT_CLASSIFY_LOW) {
            male_alt = block_sum(male_alt, sh.wave_u);
            female_alt = block_sum(female_alt, sh.wave_u);
            const uint32_t pick = !h.sex ? 0u : male_alt > female_alt ? 1u : 2u;
            if (tid == 0) sh.counter = 0;
            __syncthreads();
            uint32_t n_alt = 0;
            for (uint32_t s = tid; s < n; s += kClassifyBlock) {
                if (excluded[s]) continue;
                const uint32_t list = low_list(sh.gt[s], pick, male[s] == 1, female[s] == 1);
                n_alt += list == 2;
                if (list != 1) continue;
                Sample sm;
                parse_sample(p, starts[s], starts[s + 1] - 1, h, sm);
                const uint32_t at = atomicAdd(&sh.counter, 1u);
                if (at < kCapacity) sh.keys[at] = key_of(sm.cn);
            }
            __syncthreads();
            r.n_ref = sh.counter < kCapacity ? sh.counter : kCapacity;
            r.n_alt = block_sum(n_alt, sh.wave_u);
            if (r.n_ref) {
                uint32_t m = 1;
                while (m < r.n_ref) m <<= 1;
                for (uint32_t i = r.n_ref + tid; i < m; i += kClassifyBlock) sh.keys[i] = ~0ull;
                __syncthreads();
                classify_sort(sh.keys, m);
                r.median = median_sorted(sh.keys, r.n_ref);
                __syncthreads();
                for (uint32_t i = tid; i < r.n_ref; i += kClassifyBlock) {
                    const double dv = value_of(sh.keys[i]) - r.median;
                    sh.keys[i] = key_of(dv < 0 ? -dv : dv);
                }
                __syncthreads();
                classify_sort(sh.keys, m);
                r.mad = median_sorted(sh.keys, r.n_ref);
                uint32_t q = 0;
                for (uint32_t s = tid; s < n; s += kClassifyBlock) {
                    if (excluded[s] || low_list(sh.gt[s], pick, male[s] == 1, female[s] == 1) != 2) continue;
                    Sample sm;
                    parse_sample(p, starts[s], starts[s + 1] - 1, h, sm);
                    q += supports(sm.cn, r.median, r.mad, del);
                }
                r.quorum = block_sum(q, sh.wave_u);
            }
            finish_low(r);
        } else {
            const bool has_cn = h.key_at[kCn] != kNone;
            double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
            bool distinct = false;
            if (has_cn) {
                double x_hi = -HUGE_VAL, x_lo = -HUGE_VAL, y_hi = -HUGE_VAL, y_lo = -HUGE_VAL;     // (the minima as maxima of -v)
                uint32_t count = 0;
                for (uint32_t s = tid; s < n; s += kClassifyBlock) {
                    Sample sm;
                    parse_sample(p, starts[s], starts[s + 1] - 1, h, sm);
                    if (!sm.has_ab) continue;
                    const double y = h.sex && male[s] == 1 ? sm.cn * 2.0 : sm.cn;
                    ++count;
                    sx += sm.ab;
                    sy += y;
                    x_hi = sm.ab > x_hi ? sm.ab : x_hi;
                    x_lo = -sm.ab > x_lo ? -sm.ab : x_lo;
                    y_hi = y > y_hi ? y : y_hi;
                    y_lo = -y > y_lo ? -y : y_lo;
                }
                r.n_regressed = block_sum(count, sh.wave_u);
                sx = block_sum(sx, sh.wave_d);
                sy = block_sum(sy, sh.wave_d);
                x_hi = block_max(x_hi, sh.wave_d);
                x_lo = -block_max(x_lo, sh.wave_d);
                y_hi = block_max(y_hi, sh.wave_d);
                y_lo = -block_max(y_lo, sh.wave_d);
                distinct = r.n_regressed > 0 && x_lo < x_hi && y_lo < y_hi;
                if (distinct) {
                    const double mx = sx / (double)r.n_regressed, my = sy / (double)r.n_regressed;
                    for (uint32_t s = tid; s < n; s += kClassifyBlock) {
                        Sample sm;
                        parse_sample(p, starts[s], starts[s + 1] - 1, h, sm);
                        if (!sm.has_ab) continue;
                        const double y = h.sex && male[s] == 1 ? sm.cn * 2.0 : sm.cn;
                        const double dx = sm.ab - mx, dy = y - my;
                        sxx += dx * dx;
                        syy += dy * dy;
                        sxy += dx * dy;
                    }
                }
                sxx = block_sum(sxx, sh.wave_d);
                syy = block_sum(syy, sh.wave_d);
                sxy = block_sum(sxy, sh.wave_d);
            }
            finish_high(r, has_cn, distinct, sxx, syy, sxy, del, pr);
        }
        if (tid == 0) results[j] = r;
    }
}

}  // namespace svt

#endif  // SVT_VCF_CLASSIFY_KERNEL_H

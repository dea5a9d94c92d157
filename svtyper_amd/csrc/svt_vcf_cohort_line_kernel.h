// svt_vcf_cohort_line_kernel.h -- svt_vcf_cohort_line.h on the device (gfx950): what the kernels with ONE WORKGROUP OF 256 LANES
// PER LINE share (svt_vcf_classify_kernel.h, svt_vcf_update_info_kernel.h), in front of their passes over the samples.
//
//   line      the line-table entry, checked against the text's length (an entry outside the text reads as an empty line)
//   head      once per line: wavefront 0 finds the first nine tabs, 64 bytes a step (a ballot, a lane stores the tab it holds into
//             LDS); lane 0 runs the rule's check_head on them (INFO, the long column, is read by that one lane at most) and the
//             result is broadcast through LDS
//   starts    the bytes behind the ninth tab in 16-byte pieces, aligned in memory, a lane each and 256 side by side: one 128-bit
//             load where the piece lies inside the text (bytes in front of the column and behind the line are masked away), byte by
//             byte where it does not (the first piece of a block's first line, the last of its last), the tabs as a 16-bit mask,
//             an exclusive scan over the workgroup (shuffles inside a wavefront, the four totals through LDS, the count carried
//             from step to step), and every lane writes where the columns behind its tabs begin into LDS.  One pass
//   block_*   a value per lane -> the workgroup's: an xor butterfly per wavefront, the four results through LDS
// Every load is checked against its line's length, which is checked against the text's; every LDS index against the capacity.
// No scratch memory, no atomics, no inline assembly.
#ifndef SVT_VCF_COHORT_LINE_KERNEL_H
#define SVT_VCF_COHORT_LINE_KERNEL_H

#include "svt_vcf_cohort_line.h"

namespace svt {

constexpr int kCohortBlock = (int)cohort::kBlock;

// the LDS of the head and starts phases: a kernel's shared struct holds one, of its Head and its capacity
template <class Head, uint32_t Capacity>
struct CohortLineShared {
    uint32_t starts[Capacity + 1];                  // starts[n]: behind the line's end, as if a tab stood there
    Head head;
    uint32_t tab[9], n_tabs;
    uint32_t scan[2][4];
};

// line j of the table: where it begins, `size` its length
__device__ __forceinline__ const uint8_t* cohort_line(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t j, uint64_t& size)
{
    uint64_t off = lines[j].off;
    size = lines[j].len;
    if (off > len || size > len - off) off = size = 0;
    return text + off;
}

// the head of the line p[0, size), once: check(n, too_long, tabs, head) is the rule's
template <class Shared, class Check>
__device__ __forceinline__ auto cohort_head(Shared& sh, const uint8_t* p, uint64_t size, Check check) -> decltype(sh.head)
{
    const uint32_t lane = threadIdx.x & 63, n_line = cohort::stripped_length(p, size);
    if (threadIdx.x < 64) {
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
    if (threadIdx.x == 0) {
        cohort::Tabs t;
        t.count = sh.n_tabs;
#pragma unroll
        for (uint32_t c = 0; c < 9; ++c) t.tab[c] = c < t.count ? sh.tab[c] : n_line;
        decltype(sh.head) scanned;
        check(n_line, size > cohort::kMaxLine, t, scanned);
        sh.head = scanned;
    }
    __syncthreads();
    return sh.head;
}

// bit k: byte k of the word is a tab
__device__ __forceinline__ uint32_t cohort_tabs(uint32_t word)
{
    const uint32_t t = word ^ 0x09090909u, nonzero = ((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t, z = ~nonzero & 0x80808080u;
    return ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
}

// Where the sample columns of the line p[0, h.n) begin.  Returns their number; where that is n (1 .. the capacity: the caller
// has checked it), sh.starts[0 .. n] hold where they begin and the sentinel, behind a barrier
template <class Shared>
__device__ __forceinline__ uint32_t cohort_starts(Shared& sh, const uint8_t* text, uint64_t len, const uint8_t* p, const cohort::Head& h, uint32_t n)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t span = h.n - h.samples_b;
    const uintptr_t a_text = (uintptr_t)text, a_line = (uintptr_t)p, a_first = a_line + h.samples_b, a_0 = a_first & ~(uintptr_t)15;
    const uint32_t n_chunks = span ? (uint32_t)((a_first + span - a_0 + 15) >> 4) : 0;
    uint32_t carried = 0;
    for (uint32_t base = 0, step = 0; base < n_chunks; base += kCohortBlock, ++step) {
        const uint32_t c = base + tid;
        uint32_t m = 0;
        int64_t at_0 = 0;                           // where the piece's first byte lies in the line (the first piece: maybe in front of the column)
        if (c < n_chunks) {
            const uintptr_t a_c = a_0 + ((uintptr_t)c << 4);
            at_0 = (int64_t)a_c - (int64_t)a_line;
            const int64_t lo64 = (int64_t)h.samples_b - at_0, hi64 = (int64_t)h.n - at_0;
            const uint32_t lo = lo64 > 0 ? (uint32_t)lo64 : 0u, hi = hi64 < 16 ? (uint32_t)hi64 : 16u;
            if (a_c >= a_text && a_c + 16 <= a_text + len) {
                const uint4 w = *reinterpret_cast<const uint4*>(a_c);
                m = cohort_tabs(w.x) | cohort_tabs(w.y) << 4 | cohort_tabs(w.z) << 8 | cohort_tabs(w.w) << 12;
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
        __syncthreads();                            // (the two rows in turn: a wavefront two steps ahead has passed the barrier between)
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
    const uint32_t columns = span ? carried + 1 : 0u;
    if (columns == n && tid == 0) {
        sh.starts[0] = h.samples_b;
        sh.starts[n] = h.n + 1;
    }
    __syncthreads();
    return columns;
}

// ---- a value per lane -> the workgroup's, in every lane: `wave` holds four values
template <class T, class Join>
__device__ __forceinline__ T block_join(T v, T* wave, Join join)
{
    for (int d = 32; d; d >>= 1) v = join(v, (T)__shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = v;
    __syncthreads();
    const T total = join(join(wave[0], wave[1]), join(wave[2], wave[3]));
    __syncthreads();
    return total;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* wave)
{
    return block_join(v, wave, [](uint32_t a, uint32_t b) { return a + b; });
}

__device__ __forceinline__ uint32_t block_or(uint32_t v, uint32_t* wave)
{
    return block_join(v, wave, [](uint32_t a, uint32_t b) { return a | b; });
}

// the sum in the order of classify::Tree: (w0 + w1) + (w2 + w3)
__device__ __forceinline__ double block_sum(double v, double* wave)
{
    return block_join(v, wave, [](double a, double b) { return a + b; });
}

// the maximum (of -v: the minimum); no NaN comes here
__device__ __forceinline__ double block_max(double v, double* wave)
{
    return block_join(v, wave, [](double a, double b) { return b > a ? b : a; });
}

}  // namespace svt

#endif  // SVT_VCF_COHORT_LINE_KERNEL_H

// svt_bcf_kernel.h -- svt_bcf.h on the device (gfx950): VCF text in HBM and its line table -> BCF2.2 records.
//
// Two passes over the lines in written order (order[j]: the line that becomes record j), bcf::encode_line in both:
//   svt_bcf_measure_kernel   one lane per line, a counting sink: the record's sizes, the span's fields, a refusal with its kind,
//                            and the mark of a float outside the device envelope (bcf::Measure, 32 bytes per line)
//   (the host)               settles the marked lines with strtod, takes the lowest refused line number, and sums the sizes:
//                            where record j begins is an exclusive prefix sum, nothing is claimed with an atomic
//   svt_bcf_write_kernel     one lane per line, a storing sink over the record's own bytes; marked lines are left to the host
//                            twin, which writes those records into the same buffer
// The work split: a lane owns a line from its first byte to its last, whatever its shape.  A line is read byte by byte by its
// lane and its columns lie at data-dependent places, so neighbouring lanes do not share cache lines in a useful way either
// way; what keeps the machine busy is lines in flight.  A workgroup is one wavefront (64 lines), so that a text of a few
// thousand lines still spreads over the CUs.  The individual part of a joint line (n_sample x 15 values) is walked once per
// FORMAT key by the line's one lane: the walk is serial in the sample count.  The dictionaries are read through the caches
// from HBM (a few hundred bytes, every lane the same tables): not staged in LDS.
// Every load is checked against the line's length, which the kernels check against the text's; every store goes through
// bcf::Sink, which checks it against the record's size, which the kernels check against the output's.
#ifndef SVT_BCF_KERNEL_H
#define SVT_BCF_KERNEL_H

#include "svt_bcf.h"

namespace svt {

constexpr int kBcfBlock = 64;

// line order[j] of the table inside the text: its bytes, or false
__device__ __forceinline__ bool bcf_line(const svt_tbx_line* __restrict__ lines, uint64_t n_lines, uint64_t len, uint64_t i, uint64_t& off, uint64_t& size)
{
    if (i >= n_lines) return false;
    off = lines[i].off;
    size = lines[i].len;
    return off <= len && size <= len - off;
}

__global__ __launch_bounds__(kBcfBlock) void svt_bcf_measure_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                    uint64_t n_lines, const uint64_t* __restrict__ order, uint64_t n, const bcf::Dict d,
                                                                    bcf::Measure* __restrict__ measures)
{
    for (uint64_t j = (uint64_t)blockIdx.x * kBcfBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBcfBlock) {
        bcf::Measure m;
        uint64_t off = 0, size = 0;
        if (bcf_line(lines, n_lines, len, order[j], off, size)) {
            bcf::Sink count{nullptr, 0, 0};
            bcf::encode_line(d, text + off, size, true, count, m);
        } else {                                    // (not this launch's table)
            m.l_shared = m.l_indiv = m.at = m.host = m.beg = m.end = 0;
            m.tid = -1;
            m.kind = SVT_BCF_KIND_COLUMNS;
        }
        measures[j] = m;
    }
}

// rec_off[0 .. n]: where the records begin in out[0, out_len)
__global__ __launch_bounds__(kBcfBlock) void svt_bcf_write_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                  uint64_t n_lines, const uint64_t* __restrict__ order, uint64_t n, const bcf::Dict d,
                                                                  const bcf::Measure* __restrict__ measures, const uint64_t* __restrict__ rec_off,
                                                                  uint8_t* __restrict__ out, uint64_t out_len)
{
    for (uint64_t j = (uint64_t)blockIdx.x * kBcfBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBcfBlock) {
        bcf::Measure m = measures[j];
        if (m.kind || m.host) continue;
        const uint64_t at = rec_off[j], next = rec_off[j + 1];
        uint64_t off = 0, size = 0;
        if (at > next || next > out_len || next - at != bcf::record_bytes(m) || !bcf_line(lines, n_lines, len, order[j], off, size)) continue;
        bcf::Sink store{out + at, next - at, 0};
        bcf::encode_line(d, text + off, size, true, store, m);
    }
}

}  // namespace svt

#endif  // SVT_BCF_KERNEL_H

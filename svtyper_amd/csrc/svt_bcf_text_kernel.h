// svt_bcf_text_kernel.h -- svt_bcf_text.h on the device (gfx950): a chunk of BCF2.2 records in HBM -> their VCF lines.
//
// Two passes over the chunk's records, the rule of svt_bcf_text.h in both:
//   svt_bcf_text_measure_kernel   a counting sink: one text length, one refusal kind and one mark (a float outside the device
//                                 envelope) per record (bcftext::TextMeasure, 16 bytes)
//   (the host)                    measures the marked records with snprintf, takes the lowest refused record, and sums the
//                                 lengths: where line j begins is an exclusive prefix sum, nothing is claimed with an atomic
//   svt_bcf_text_write_kernel     a storing sink over the line's own bytes; marked records are left to the host twin
// The work split: ONE WAVEFRONT PER RECORD, LANES OVER SAMPLES.  A record's individual part is field-major (per FORMAT key all
// samples side by side at a fixed stride), a VCF line is sample-major: the decode is a transpose.  Every lane runs
// shared_text -- the same loads in every lane, one instruction stream, so the shared part is walked once per record by its
// wave -- and only lane 0's sink has a buffer.  Sample s then belongs to lane s % 64, in strides of 64: a lane walks the
// record's few FORMAT descriptors (uniform loads again), finds its sample's values at an O(1) place per key and measures its
// column; an inclusive scan over the wave, with a carry from stride to stride, gives each column its place in the line.  The
// write kernel measures the columns again in front of the stores (the same walk, a counting sink): no per-column sizes are
// kept between the kernels.  A workgroup is four waves, four records; the dictionaries are read through the caches.
// Every load is checked against the record's l_shared / l_indiv, which shared_text checks against the record's length, which
// the kernels check against the chunk's; every store goes through bcf::Sink, whose capacity is the column's measured length
// clipped to the line's, which the kernels check against the output's.
#ifndef SVT_BCF_TEXT_KERNEL_H
#define SVT_BCF_TEXT_KERNEL_H

#include "svt_bcf_text.h"

namespace svt {

namespace bcftext {
struct TextMeasure {
    uint64_t len;
    uint32_t kind, host;
};
}  // namespace bcftext

constexpr int kBcfTextBlock = 256, kBcfTextWaves = kBcfTextBlock / 64;

__device__ __forceinline__ uint64_t bcf_text_wave_scan(uint64_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// record j of the chunk inside stream[0, len): its bytes, or false
__device__ __forceinline__ bool bcf_text_record(const uint64_t* __restrict__ rec_off, uint64_t len, uint64_t j, uint64_t& off, uint64_t& size)
{
    off = rec_off[j];
    const uint64_t next = rec_off[j + 1];
    size = next - off;
    return off <= next && next <= len;
}

// rec_off[0 .. n]: where the records begin in stream[0, len)
__global__ __launch_bounds__(kBcfTextBlock) void svt_bcf_text_measure_kernel(const uint8_t* __restrict__ stream, uint64_t len,
                                                                             const uint64_t* __restrict__ rec_off, uint64_t n, const bcftext::TextDict d,
                                                                             bcftext::TextMeasure* __restrict__ measures)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * kBcfTextWaves + threadIdx.x / 64; j < n; j += (uint64_t)gridDim.x * kBcfTextWaves) {
        bcftext::TextMeasure m{0, SVT_BCF_TEXT_KIND_TRUNCATED, 0};
        uint64_t off = 0, size = 0;
        if (bcf_text_record(rec_off, len, j, off, size)) {
            bcf::Sink count{nullptr, 0, 0};
            bcftext::Shape sh;
            m.kind = bcftext::shared_text(d, stream + off, size, true, count, sh);
            if (!m.kind) {
                uint64_t total = count.n;
                uint32_t outside = sh.outside;
                for (uint32_t base = 0; sh.n_fmt && base < sh.n_sample; base += 64) {
                    bcf::Sink column{nullptr, 0, 0};
                    if (base + lane < sh.n_sample) bcftext::sample_text(d, stream + off, sh, base + lane, true, column, outside);
                    total += (uint64_t)__shfl((unsigned long long)bcf_text_wave_scan(column.n, lane), 63);
                }
                m.len = total + 1;
                m.host = __any((int)outside) ? 1u : 0u;
            }
        }
        if (lane == 0) measures[j] = m;
    }
}

// text_off[0 .. n]: where the lines begin in out[0, out_len)
__global__ __launch_bounds__(kBcfTextBlock) void svt_bcf_text_write_kernel(const uint8_t* __restrict__ stream, uint64_t len,
                                                                           const uint64_t* __restrict__ rec_off, uint64_t n, const bcftext::TextDict d,
                                                                           const bcftext::TextMeasure* __restrict__ measures,
                                                                           const uint64_t* __restrict__ text_off, uint8_t* __restrict__ out, uint64_t out_len)
{
    const int lane = threadIdx.x & 63;
    for (uint64_t j = (uint64_t)blockIdx.x * kBcfTextWaves + threadIdx.x / 64; j < n; j += (uint64_t)gridDim.x * kBcfTextWaves) {
        const bcftext::TextMeasure m = measures[j];
        if (m.kind || m.host) continue;
        const uint64_t at = text_off[j], next = text_off[j + 1];
        uint64_t off = 0, size = 0;
        if (at > next || next > out_len || next - at != m.len || !bcf_text_record(rec_off, len, j, off, size)) continue;
        const uint64_t room = next - at;
        bcf::Sink head{lane == 0 ? out + at : nullptr, room, 0};
        bcftext::Shape sh;
        if (bcftext::shared_text(d, stream + off, size, true, head, sh)) continue;
        uint64_t carry = head.n;
        uint32_t outside = 0;
        for (uint32_t base = 0; sh.n_fmt && base < sh.n_sample; base += 64) {
            const bool mine = base + lane < sh.n_sample;
            bcf::Sink column{nullptr, 0, 0};
            if (mine) bcftext::sample_text(d, stream + off, sh, base + lane, true, column, outside);
            const uint64_t behind = bcf_text_wave_scan(column.n, lane), place = carry + behind - column.n;
            if (mine && place < room) {
                bcf::Sink store{out + at + place, column.n < room - place ? column.n : room - place, 0};
                bcftext::sample_text(d, stream + off, sh, base + lane, true, store, outside);
            }
            carry += (uint64_t)__shfl((unsigned long long)behind, 63);
        }
        if (lane == 0 && carry < room) out[at + carry] = '\n';
    }
}

}  // namespace svt

#endif  // SVT_BCF_TEXT_KERNEL_H

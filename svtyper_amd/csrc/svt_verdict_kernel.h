// svt_verdict_kernel.h -- the per-record verdicts behind `svtyper -w` (svt_batch_verdicts, include/svtyper_hip.h): which of the
// reference's tagging branches a fragment's record takes (classic.py:317-408) and which XV tag each of them sets
// (parsers.py:771-782,1218-1228).  The small-deletion gate and p_concordant exist on the device only (svt_unit_math.h:
// pair_gate_and_concordance, the function the general-mode pass calls); the host has the geometry and nothing else.
// Internal header of libsvtyper_hip.so (single translation unit: svtyper_hip.hip).
//
// Not a hot kernel: it runs once per chunk of a `-w` run and never otherwise.  One wavefront per unit, the lanes stride over the
// unit's records (one 16-byte load, one byte store per record), a grid-stride loop over the units; every table is read where
// the batch uploaded it (pm, wtab, LibDesc[], Bin[] through ordinary pointers: L2), each library through its own descriptor --
// so the bytes do not depend on the mode the batch's pass runs in, and any library index a record can name (16 bits) works.
#ifndef SVT_VERDICT_KERNEL_H
#define SVT_VERDICT_KERNEL_H

#include "svt_unit_math.h"

namespace svt {

constexpr int kVerdictBlock = 256;   // four wavefronts = four units per workgroup and step

struct VerdictArgs {
    const uint4* records;        // the canonical records of the resident batch
    const uint64_t* rec_offset;  // n_units + 1
    const svt_unit* units;
    const double* pm;            // prob_mapq[256]
    const PairWeights* wtab;     // the paired-end decision table (32)
    const LibDesc* libs;
    const Bin* bins;
    uint8_t* out;                // one byte per record
    uint64_t n_records;          // records and bytes of `out`: no offset is followed beyond it
    uint32_t n_units, n_libs;
};

__global__ __launch_bounds__(kVerdictBlock) void svt_verdict_kernel(const VerdictArgs a)
{
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint32_t waves_per_wg = kVerdictBlock / kWave;
    const uint32_t n_waves = gridDim.x * waves_per_wg;
    Tables t;
    t.pm = a.pm;
    t.wtab = a.wtab;
    t.libs = a.libs;
    t.bins = a.bins;
    for (uint32_t u = blockIdx.x * waves_per_wg + threadIdx.x / kWave; u < a.n_units; u += n_waves) {
        const svt_unit U = a.units[u];
        const uint64_t r0 = a.rec_offset[u], r1 = min(a.rec_offset[u + 1], a.n_records);
        const bool skipped = (U.flags & SVT_UNIT_SKIP) != 0;     // classic.py:282-284: no read of the unit is looked at
        LaneCtx c{};
        c.is_del = U.svtype == SVT_SVTYPE_DEL;
        c.del16 = c.is_del ? 16u : 0u;
        c.var_length = U.var_length;
        c.pos_delta_d = (double)U.pos_delta;
        for (uint64_t r = r0 + lane; r < r1; r += kWave) {
            const uint4 w = a.records[r];
            uint32_t v = 0u;
            if (!skipped) {
                // a split candidate counts -- and is tagged A -- when p_alt > 0 (classic.py:324,330)
                const double p_seq = (t.pm[w.z & 0xffu] + t.pm[(w.z >> 8) & 0xffu]) * 0.5;
                const double p_clip = (t.pm[(w.z >> 16) & 0xffu] + t.pm[w.z >> 24]) * 0.5;
                v |= p_seq > 0.0 ? 16u : 0u;
                v |= p_clip > 0.0 ? 32u : 0u;
                const bool first = (w.w & SVT_REC_CONTINUATION) == 0u;
                if (first && (w.w & SVT_REC_HAS_PAIR)) {
                    uint32_t f3 = w.w & 7u;
                    const bool p_conc = pair_gate_and_concordance(w.x, f3, min(SVT_REC_LIB(w.w), a.n_libs - 1u), t, c);
                    const double pp = t.pm[w.y & 0xffu] * t.pm[(w.y >> 8) & 0xffu];
                    // classic.py:359-380: p_alt = (1 - p_conc) * pmA * pmB for DEL, pmA * pmB otherwise = pp * w_alt
                    const PairWeights pw = t.wtab[f3 | (p_conc ? 8u : 0u) | c.del16];
                    if (f3 & 1u) v |= 1u | (pp * pw.w_alt > 0.0 ? 2u : 0u);
                    // classic.py:398-408: tag_span(1 - p_conc)
                    const bool ra = (f3 & 2u) != 0u, rb = (f3 & 4u) != 0u;
                    if ((ra || rb) && (!(ra && rb) || c.is_del)) v |= 4u | (p_conc ? 0u : 8u);
                }
            }
            a.out[r] = (uint8_t)v;
        }
    }
}

}  // namespace svt

#endif  // SVT_VERDICT_KERNEL_H

// svt_dump_kernel.h -- the evidence dump of `svtyper -w` on the device (gfx950): svt_dump_rules.h over the source rows the walk's
// write pass left (svt_evidence_src_kernel / svt_evidence_deep_src_kernel, svt_evidence_kernel.h), the verdict bytes of
// svt_verdict_kernel and the arena, all of them where they already lie in HBM.  Internal header of libsvtyper_hip.so (single
// translation unit: svtyper_hip.hip).
//
// Two launches in the count / host scan / write idiom:
//   svt_dump_size_kernel   one wavefront per unit, the lanes striding over the unit's fragments: the decision per fragment and
//                          the tag walk of its reads; per read slot (two per row) the output length (0 = not written) and the
//                          tag state; the wave adds up the unit's bytes (shuffles) and ands "inside the envelope".
//   (host)                 the prefix sum of the units' bytes; a unit outside the envelope gets none.
//   svt_dump_write_kernel  one workgroup per unit: a prefix sum over the unit's slot lengths places each read, then each read is
//                          copied by one of the four wavefronts -- dwords where source and destination agree mod 4, bytes
//                          elsewhere -- and gets its XV field.
// Neither is hot (they run once per chunk of a `-w` run and never otherwise) and neither is tuned.  Plain vector loads and stores,
// no atomics, no floats; what lands where is decided by the rows and the verdicts, not by the schedule.  A unit that is
// skipped or empty has no rows and writes nothing; a unit the host reader spliced in (unit_host) has no source rows: it is
// passed by.
#ifndef SVT_DUMP_KERNEL_H
#define SVT_DUMP_KERNEL_H

#include "svt_dump_rules.h"
#include "svt_evidence_kernel.h"

namespace svt {

constexpr int kDumpBlock = 256;
static_assert(kDumpBlock % kWave == 0, "whole wavefronts");

struct DumpWaveCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x & (kWave - 1u); }
    static __device__ __forceinline__ uint32_t lanes() { return kWave; }
    static __device__ __forceinline__ void sync() {}
};
struct DumpBlockCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kDumpBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

struct DumpArgs {
    const uint8_t* arena;
    uint64_t arena_len;
    const ew::SrcRow* rows;      // one per record of the batch
    const uint8_t* verdicts;     // one per record of the batch
    const uint64_t* rec_offset;  // n_units + 1
    const uint8_t* unit_host;    // n_units: 1 = the host reader's records, no source rows
    uint32_t n_units;
    uint32_t* slot_len;          // 2 per record
    uint8_t* slot_state;         // 2 per record
    uint32_t* slot_off;          // 2 per record: where the slot's read lies in its unit's bytes (the write launch's own)
    uint64_t* unit_bytes;        // size launch: per unit
    uint32_t* unit_reads;        // size launch: per unit, reads written
    uint32_t* unit_outside;      // size launch: per unit, 1 = outside the dump's envelope
    const uint64_t* unit_offset; // write launch: n_units + 1
    uint8_t* bytes;
    uint32_t* error;             // write launch: set when a read does not give the bytes it was sized for
};

__device__ __forceinline__ dr::Unit dump_unit(const DumpArgs& a, uint32_t u)
{
    const uint64_t r0 = a.rec_offset[u], r1 = a.rec_offset[u + 1];
    dr::Unit U;
    U.arena = a.arena;
    U.arena_len = a.arena_len;
    U.rows = a.rows + r0;
    U.verdicts = a.verdicts + r0;
    U.n_rows = (uint32_t)(r1 - r0);
    U.slot_len = a.slot_len + 2 * r0;
    U.slot_state = a.slot_state + 2 * r0;
    return U;
}

__global__ __launch_bounds__(kDumpBlock) void svt_dump_size_kernel(const DumpArgs a)
{
    const uint32_t u = blockIdx.x * (kDumpBlock / kWave) + threadIdx.x / kWave;
    if (u >= a.n_units) return;                                   // (the same for every lane of the wavefront)
    uint64_t bytes = 0;
    uint32_t reads = 0;
    bool ok = true;
    if (!a.unit_host[u]) ok = dr::size_unit<DumpWaveCtx>(dump_unit(a, u), bytes, reads);
    uint32_t lo = (uint32_t)bytes, hi = (uint32_t)(bytes >> 32), bad = ok ? 0u : 1u;
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const uint32_t lo2 = __shfl_xor(lo, d), hi2 = __shfl_xor(hi, d);
        const uint64_t sum = (((uint64_t)hi << 32) | lo) + (((uint64_t)hi2 << 32) | lo2);
        lo = (uint32_t)sum;
        hi = (uint32_t)(sum >> 32);
        bad |= __shfl_xor(bad, d);
        reads += __shfl_xor(reads, d);
    }
    if (DumpWaveCtx::lane() == 0) {
        a.unit_bytes[u] = bad ? 0ull : (((uint64_t)hi << 32) | lo);
        a.unit_outside[u] = bad;
        a.unit_reads[u] = bad ? 0u : reads;
    }
}

__global__ __launch_bounds__(kDumpBlock) void svt_dump_write_kernel(const DumpArgs a)
{
    __shared__ uint32_t partial[kDumpBlock];
    const uint32_t u = blockIdx.x;
    if (u >= a.n_units || a.unit_host[u]) return;                 // (the same for every lane of the workgroup)
    const uint64_t b0 = a.unit_offset[u], total = a.unit_offset[u + 1] - b0;
    const dr::Unit U = dump_unit(a, u);
    if (total == 0 || U.n_rows == 0) return;
    const uint32_t n_slots = 2 * U.n_rows;
    uint32_t* slot_off = a.slot_off + 2 * a.rec_offset[u];
    dr::place_slots<DumpBlockCtx>(U.slot_len, slot_off, n_slots, partial);
    for (uint32_t k = threadIdx.x / kWave; k < n_slots; k += kDumpBlock / kWave) {
        const uint32_t len = U.slot_len[k];
        if (!len) continue;
        const bool fits = (uint64_t)slot_off[k] + len <= total;
        if (!fits || !dr::emit_read<DumpWaveCtx>(U.arena, U.arena_len, U.rows[k / 2].rec[k & 1], U.slot_state[k], a.bytes + b0 + slot_off[k], len))
            if (DumpWaveCtx::lane() == 0) a.error[0] = 1u;
    }
}

}  // namespace svt

#endif  // SVT_DUMP_KERNEL_H

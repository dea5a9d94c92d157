// svt_evidence_kernel.h -- the walk of svt_evidence_walk.h on the device (gfx950): inflated BAM bytes in HBM -> evidence records
// and their CSR in HBM, in the layout svt_batch_create would have uploaded.  No evidence crosses PCIe.
//
// One workgroup of 256 lanes (four wave64) per (breakpoint, sample) unit; the per-unit state (ew::UnitScratch) is LDS.
//   * lane 0 follows the block_size chain of the unit's ranges, 256 records at a time; the 256 lanes decode those records side by
//     side (core fields, reference end from the CIGAR, pysam's overlap rule, the flag filters, the tag walk, RG -> library,
//     aligned intervals, the SA entry) into LDS summaries; lane 0 then applies what depends on arrival order (the counts of the
//     max_reads rules, the slot of every kept read);
//   * the kept reads are ranked by (query name, arrival) -- a rank sort over an 8-byte key in LDS (the bytes behind the names'
//     common prefix), whole names compared from HBM only between equal keys;
//   * runs of one name are fragments: repeated (name, flag) dropped, max(1, ceil(primaries / 2), |seq|, |clip|) rows each,
//     every row through svt_geometry_math.h into its 16-byte record.
// Unit sizes are not known in advance: the kernel runs twice -- <false> counts rows per unit (and reports the unit's status),
// the host scans the counts into rec_offset (and gives the out-of-envelope units their place), <true> walks again and writes
// each unit's records where they belong.  The records of host-recomputed units are scattered in by svt_evidence_scatter_kernel.
//
// Capacities and the LDS they cost (ew::UnitScratch, 72 232 bytes: two workgroups per CU of 160 KiB; with 1 536 reads it would
// be one):
//   reads per unit  1 024 x 52-byte summary = 53 248   (measured with svt_bam_evidence_walk_host: the fixture's 211 units keep 617 at most; 30x units ~530 on
//                                                       average; svtyper-sso's --max_reads 1000 is per window)
//   batch           256 x (52-byte summary + 20 bytes of offsets / counts / verdicts) = 18 944, reused after the gather for
//   sort + rows     1 024 x (8-byte key + three 16-bit arrays) = 14 336
//   name bytes      128 (compared in HBM, the cap bounds the compare), CIGAR operations 256 (walked in HBM), SA entries 8 /
//                   1 024 bytes: none of them costs LDS
// Everything is written with ordinary vector stores from plain C++.
#ifndef SVT_EVIDENCE_KERNEL_H
#define SVT_EVIDENCE_KERNEL_H

#include "svt_evidence_walk.h"

namespace svt {

constexpr int kEvidenceBlock = 256;

struct EvidenceDevCtx {
    static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
    static __device__ __forceinline__ uint32_t lanes() { return kEvidenceBlock; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};

struct EvidenceArgs {
    ew::Params P;
    uint32_t n_units;
    uint32_t* status;            // per unit: ew::EW_*
    uint32_t* n_rows;            // per unit: records (0 unless EW_OK)
    uint32_t* n_reads;           // per unit: kept reads
    const uint64_t* rec_offset;  // <true>: where the unit's records go
    uint4* records;
};

template <bool kWrite>
__global__ __launch_bounds__(kEvidenceBlock) void svt_evidence_kernel(const EvidenceArgs a)
{
    extern __shared__ __align__(16) unsigned char svt_evidence_lds[];
    ew::UnitScratch& S = *reinterpret_cast<ew::UnitScratch*>(svt_evidence_lds);
    const uint32_t u = blockIdx.x;
    if (u >= a.n_units) return;
    if (kWrite && (a.status[u] != ew::EW_OK || a.n_rows[u] == 0)) return;      // (the same for every lane of the workgroup)
    static_assert(sizeof(Record4) == sizeof(uint4), "a record is four words");
    Record4* out = kWrite ? reinterpret_cast<Record4*>(a.records + a.rec_offset[u]) : nullptr;
    ew::walk_unit<EvidenceDevCtx>(a.P, u, S, out);
    if (!kWrite && threadIdx.x == 0) {
        a.status[u] = S.status;
        a.n_rows[u] = S.status == ew::EW_OK ? S.n_rows : 0u;
        a.n_reads[u] = S.n_reads;
    }
}

// records of the units the host recomputed: `src` holds them side by side, unit k's `count[k]` records go to `dst_off[k]`
__global__ __launch_bounds__(kEvidenceBlock) void svt_evidence_scatter_kernel(const uint4* __restrict__ src, const uint64_t* __restrict__ src_off,
                                                                              const uint64_t* __restrict__ dst_off, uint32_t n, uint4* __restrict__ dst)
{
    const uint32_t k = blockIdx.x;
    if (k >= n) return;
    const uint64_t s0 = src_off[k], cnt = src_off[k + 1] - s0, d0 = dst_off[k];
    for (uint64_t i = threadIdx.x; i < cnt; i += kEvidenceBlock) dst[d0 + i] = src[s0 + i];
}

}  // namespace svt

#endif  // SVT_EVIDENCE_KERNEL_H

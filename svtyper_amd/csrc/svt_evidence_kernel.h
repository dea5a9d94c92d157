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
//
// Two tiers of kept reads per unit.  svt_evidence_kernel walks every unit with its tables in LDS, up to 1 024 reads; a unit
// with more comes out of its count pass as EW_READS with its true number of kept reads.  Those of up to 16 384 reads are walked
// again by svt_evidence_deep_kernel, the same walk with the tables in a slice of an HBM workspace; beyond that the unit is the
// host reader's.
//
// Capacities and the memory they cost:
//                   LDS tier (ew::UnitScratch, 72 240 bytes of LDS:   deep tier (ew::DeepScratch, 24 624 bytes of LDS, and a
//                   two workgroups per CU of 160 KiB)                 slice of ew::kDeepSliceBytes = 1 179 648 bytes of HBM)
//   reads per unit  1 024 x 52-byte summary = 53 248  LDS             16 384 x 52 = 851 968  HBM
//   batch           256 x (52-byte summary + 22 bytes of offsets /    256 x (52 + 24) = 19 456  LDS, reused by the sort for
//                   counts / verdicts) = 18 944  LDS, reused for      a tile of 2 048 x (8-byte key + 32-bit read) = 24 576
//   sort + rows     1 024 x (8-byte key + three 16-bit arrays)        16 384 x (8-byte key + three 32-bit arrays)
//                   = 14 336  LDS                                     = 327 680  HBM
//   name bytes      128 (compared in HBM, the cap bounds the compare), CIGAR operations 256 (walked in HBM), SA entries 8 /
//                   1 024 bytes: none of them costs LDS, in either tier
// (measured with svt_bam_evidence_walk_host: the fixture's 211 units keep 617 reads at most, 30x units ~530 on average;
// svtyper-sso's --max_reads 1000 is per window, classic svtyper has no limit by default.)
// The workspace holds a slice per deep workgroup, at most kDeepMaxSlices = 227 of them (<= 256 MiB); the deep kernel is
// launched with min(deep units, 227) workgroups, each taking the deep units blockIdx.x, blockIdx.x + gridDim.x, ...
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
    ew::walk_unit<EvidenceDevCtx>(a.P, u, S, S.tables(), out);
    if (!kWrite && threadIdx.x == 0) {
        a.status[u] = S.status;
        a.n_rows[u] = S.status == ew::EW_OK ? S.n_rows : 0u;
        a.n_reads[u] = S.n_reads;
    }
}

// ---- the deep tier ------------------------------------------------------------------------------------------------------------
constexpr uint64_t kDeepWorkspaceMax = 256ull << 20;
constexpr uint32_t kDeepMaxSlices = (uint32_t)(kDeepWorkspaceMax / ew::kDeepSliceBytes);
static_assert(kDeepMaxSlices == 227 && ew::kDeepSliceBytes % 8 == 0, "the slices of the deep workspace");

struct EvidenceDeepArgs {
    ew::Params P;
    uint32_t n_deep;
    const uint32_t* unit;        // per deep unit: its index in the call
    uint32_t* status;            // per deep unit: ew::EW_* (the unit's entry in EvidenceArgs::status stays EW_READS: the LDS tier passes it by)
    uint32_t* n_rows;            // per deep unit: records (0 unless EW_OK)
    const uint64_t* rec_offset;  // <true>: per unit of the call, where its records go
    uint4* records;
    uint8_t* workspace;          // gridDim.x slices of ew::kDeepSliceBytes
};

template <bool kWrite>
__global__ __launch_bounds__(kEvidenceBlock) void svt_evidence_deep_kernel(const EvidenceDeepArgs a)
{
    __shared__ ew::DeepScratch S;
    const ew::Tables<uint32_t> T = ew::deep_tables(a.workspace + (uint64_t)blockIdx.x * ew::kDeepSliceBytes);
    for (uint32_t k = blockIdx.x; k < a.n_deep; k += gridDim.x) {                  // (k is the same for every lane of the workgroup)
        if (kWrite && (a.status[k] != ew::EW_OK || a.n_rows[k] == 0)) continue;
        const uint32_t u = a.unit[k];
        Record4* out = kWrite ? reinterpret_cast<Record4*>(a.records + a.rec_offset[u]) : nullptr;
        ew::walk_unit<EvidenceDevCtx>(a.P, u, S, T, out);
        if (!kWrite && threadIdx.x == 0) {
            a.status[k] = S.status;
            a.n_rows[k] = S.status == ew::EW_OK ? S.n_rows : 0u;    // (its kept reads are the LDS tier's count: EvidenceArgs::n_reads)
        }
        __syncthreads();                                                           // (S is the next unit's from here on)
    }
}

// ---- the write pass with source rows (the evidence dump: svt_dump_kernel.h) ----------------------------------------------------
// svt_evidence_kernel<true> and svt_evidence_deep_kernel<true> with ew::walk_unit's kSrc: beside every record its ew::SrcRow, at
// the record's index.  Kernels of their own, so that the four instantiations above are what they are without the dump.
__global__ __launch_bounds__(kEvidenceBlock) void svt_evidence_src_kernel(const EvidenceArgs a, ew::SrcRow* src)
{
    extern __shared__ __align__(16) unsigned char svt_evidence_lds[];
    ew::UnitScratch& S = *reinterpret_cast<ew::UnitScratch*>(svt_evidence_lds);
    const uint32_t u = blockIdx.x;
    if (u >= a.n_units) return;
    if (a.status[u] != ew::EW_OK || a.n_rows[u] == 0) return;                    // (the same for every lane of the workgroup)
    ew::walk_unit<EvidenceDevCtx, ew::UnitScratch, true>(a.P, u, S, S.tables(), reinterpret_cast<Record4*>(a.records + a.rec_offset[u]), src + a.rec_offset[u]);
}

__global__ __launch_bounds__(kEvidenceBlock) void svt_evidence_deep_src_kernel(const EvidenceDeepArgs a, ew::SrcRow* src)
{
    __shared__ ew::DeepScratch S;
    const ew::Tables<uint32_t> T = ew::deep_tables(a.workspace + (uint64_t)blockIdx.x * ew::kDeepSliceBytes);
    for (uint32_t k = blockIdx.x; k < a.n_deep; k += gridDim.x) {                  // (k is the same for every lane of the workgroup)
        if (a.status[k] != ew::EW_OK || a.n_rows[k] == 0) continue;
        const uint32_t u = a.unit[k];
        ew::walk_unit<EvidenceDevCtx, ew::DeepScratch, true>(a.P, u, S, T, reinterpret_cast<Record4*>(a.records + a.rec_offset[u]), src + a.rec_offset[u]);
        __syncthreads();                                                           // (S is the next unit's from here on)
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

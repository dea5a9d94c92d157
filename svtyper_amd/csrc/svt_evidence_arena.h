// svt_evidence_arena.h -- what the reader (svt_reads_arena.h, a part of svt_reads.cpp) hands to the two callers of svt_evidence_walk.h: the arena of inflated
// BGZF payloads of one call with the per-unit record ranges in it, and the host recomputation of single units.  Internal C++
// (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_EVIDENCE_ARENA_H
#define SVT_EVIDENCE_ARENA_H

#include <cstdint>
#include <string>
#include <vector>

#include "svt_bgzf.h"
#include "svt_evidence_walk.h"

namespace svt {

namespace ew {

struct Arena {
    std::vector<uint8_t> bytes;            // inflated blocks; the blocks a range needs lie side by side, every block once
    std::vector<Range> ranges;
    std::vector<UnitRanges> units;         // n_units
    std::vector<NameRef> rgs, refs;
    std::vector<uint8_t> blob;             // the bytes of the read-group ids and reference names
    uint64_t records_in_ranges = 0;
    uint64_t blocks = 0;                   // BGZF blocks in `bytes`
    double build_s = 0.0;
    bool open_ranges = false;              // build_arena_open: the walk ends every window itself (Params.open_ranges)
    Params params(const svt_summarise_args* args, const svt_evidence_params* geometry) const
    {
        Params P{};
        P.arena = bytes.data();
        P.arena_len = bytes.size();
        P.ranges = ranges.data();
        P.units = units.data();
        P.windows = args->windows;
        P.bps = args->breakpoints;
        P.rgs = rgs.data();
        P.refs = refs.data();
        P.blob = blob.data();
        P.lib_flank = geometry->lib_flank;
        P.n_rgs = (uint32_t)rgs.size();
        P.n_refs = (uint32_t)refs.size();
        P.n_libs = geometry->n_libs;
        P.min_aligned = geometry->min_aligned;
        P.split_slop = geometry->split_slop;
        P.count_mode = args->count_mode;
        P.max_reads = args->max_reads;
        P.open_ranges = open_ranges ? 1u : 0u;
        return P;
    }
};

// The tier rule, for both callers of the walk: a unit that the first tier (tables of kMaxReads) left with EW_READS and its true
// number of kept reads is walked once more with the deep tier's tables when they hold that many.
inline bool deep_tier_unit(uint32_t status, uint32_t n_reads) { return status == EW_READS && n_reads <= kMaxReadsDeep; }

// The arena comes from ONE planner in svt_reads_arena.h with two routes.  Shared: the argument checks, the names, every unit's windows
// cut into index chunks on the reader's threads, the runs of blocks the ranges need, the 32-bit limit of the arena's offsets (a
// unit behind it is preset to EW_RANGE) and the ranges.  A route says how a chunk becomes a range and how a run is placed.

// The host route.  A chunk is inflated (the reader's block cache) and its records are walked up to the one that ends the fetch;
// a run's blocks are copied side by side.  0 or SVT_ERR_* with the error text set.
int build_arena(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out);

// ---- the arena without inflating on the host (inflate = "device") ---------------------------------------------------------------
// What build_arena_open leaves to its caller: the BGZF members whose ISIZE bytes make up the arena (bgzf::MemberSet: one span of
// the file per run of blocks), and `range_members[r]`: the members arena.ranges[r] lies over (first, last).
struct OpenPlan {
    bgzf::MemberSet set;
    std::vector<std::pair<uint32_t, uint32_t>> range_members;
    double index_s = 0.0;
};

// The open route.  A chunk is followed through BGZF headers only and becomes one range from its start to its end virtual offset
// (an upper bound; Params.open_ranges makes the walk stop where the fetch does); a run's blocks become `plan.set.members` out of
// one span of the file.  out.bytes is sized, not filled: bgzf::inflate_members_host or svt_inflate_kernel fills it.
int build_arena_open(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out, OpenPlan& plan);
// every unit with a range over a member whose status is not 0 gets preset = EW_RANGE; returns the number of failed members
uint64_t apply_member_status(const OpenPlan& plan, const std::vector<uint32_t>& status, Arena& out);

// the units `ids` (ascending) recomputed by the host reader: their records side by side in `records`, `counts[k]` of them for
// ids[k], `skipped[k]`.  An error is the one svt_bam_evidence reports for that unit (code returned, text set).
int host_units(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const std::vector<uint64_t>& ids,
               std::vector<svt_record>& records, std::vector<uint64_t>& counts, std::vector<uint8_t>& skipped);

}  // namespace ew
}  // namespace svt

#endif  // SVT_EVIDENCE_ARENA_H

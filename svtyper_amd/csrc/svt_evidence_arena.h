// svt_evidence_arena.h -- what the reader (svt_reads.cpp) hands to the two callers of svt_evidence_walk.h: the arena of inflated
// BGZF payloads of one call with the per-unit record ranges in it, and the host recomputation of single units.  Internal C++
// (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_EVIDENCE_ARENA_H
#define SVT_EVIDENCE_ARENA_H

#include <cstdint>
#include <string>
#include <vector>

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
    double build_s = 0.0;
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
        return P;
    }
};

// BAI lookup + BGZF inflate of every unit's windows (the reader's threads and block cache); 0 or SVT_ERR_* with the error text set
int build_arena(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out);

// the units `ids` (ascending) recomputed by the host reader: their records side by side in `records`, `counts[k]` of them for
// ids[k], `skipped[k]`.  An error is the one svt_bam_evidence reports for that unit (code returned, text set).
int host_units(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const std::vector<uint64_t>& ids,
               std::vector<svt_record>& records, std::vector<uint64_t>& counts, std::vector<uint8_t>& skipped);

}  // namespace ew
}  // namespace svt

#endif  // SVT_EVIDENCE_ARENA_H

// svt_library_arena.h -- what svt_reads_library.h (a part of svt_reads.cpp) hands to the two callers of svt_library_walk.h: the rounds of the record stream
// (members to inflate, segments in the arena they make), and the one driver both routes go through -- rounds, prefix sums, caps,
// stop rule, merge, the host scan for whatever is outside the envelope.  A route is a Backend: where the arena and the tables
// live and who runs the walk.  Internal C++ (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_LIBRARY_ARENA_H
#define SVT_LIBRARY_ARENA_H

#include <cstdint>
#include <vector>

#include "../../include/svtyper_reads.h"
#include "svt_bgzf.h"
#include "svt_evidence_arena.h"
#include "svt_library_walk.h"

namespace svt {
namespace lw {

// One round: whole BGZF members out of one span of the file (bgzf::MemberSet) and the segments of the arena they inflate to.
struct Round {
    bgzf::MemberSet set;
    std::vector<Segment> segments;
    VerifyTally* verify = nullptr;       // svt_bam_set_verify: whoever loads the round checks its members' CRC-32 and counts here
};

// the host's copies of the tables, for the merge
struct HostTables {
    uint32_t n_libs = 0;
    std::vector<uint64_t> dense_count, dense_first, read_length, in_lib;
    std::vector<Overflow> overflow;                  // the entries written (at most the capacity)
    uint32_t overflow_n = 0;                         // the entries asked for
};

struct Backend {
    virtual ~Backend() {}
    // the names and the tables (zeroed; dense_first all ones) for n_libs libraries, an overflow list of overflow_cap entries
    virtual int begin(const std::vector<ew::NameRef>& rgs, const std::vector<uint8_t>& blob, uint32_t n_libs, uint32_t overflow_cap) = 0;
    // the round's arena; member_status[k] = inf::INF_*
    virtual int load(const Round& r, std::vector<uint32_t>& member_status, svt_library_scan_stats& S) = 0;
    virtual int count(const std::vector<Segment>& segments, std::vector<SegCount>& counts) = 0;
    virtual int accumulate(const std::vector<Segment>& segments, const std::vector<SegCaps>& caps) = 0;   // caps.size() segments
    virtual int finish(HostTables& T) = 0;
};

// the whole call.  0 or SVT_ERR_* with the error text set (the host scan's, when it answered).
int scan_libraries(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts, const char* const* read_groups, int64_t num_samp,
                   uint64_t round_bytes, Backend& backend, svt_library_scan* out, svt_library_scan_stats* stats);

}  // namespace lw
}  // namespace svt

#endif  // SVT_LIBRARY_ARENA_H

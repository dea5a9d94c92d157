// svt_library_arena.h -- what svt_reads.cpp hands to the two callers of svt_library_walk.h: the rounds of the record stream
// (members to inflate, segments in the arena they make), and the one driver both routes go through -- rounds, prefix sums, caps,
// stop rule, merge, the host scan for whatever is outside the envelope.  A route is a Backend: where the arena and the tables
// live and who runs the walk.  Internal C++ (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_LIBRARY_ARENA_H
#define SVT_LIBRARY_ARENA_H

#include <cstdint>
#include <vector>

#include "../../include/svtyper_reads.h"
#include "svt_evidence_arena.h"
#include "svt_inflate.h"
#include "svt_library_walk.h"

namespace svt {
namespace lw {

// One round: the BGZF members file[span_off, span_off + span_bytes) side by side (Member.src counts from span_off, Member.dst in
// the arena) and the segments of the arena they inflate to.
struct Round {
    const uint8_t* file = nullptr;
    uint64_t span_off = 0, span_bytes = 0, arena_bytes = 0;
    std::vector<inf::Member> members;
    std::vector<Segment> segments;
    VerifyTally* verify = nullptr;       // svt_bam_set_verify: whoever loads the round checks its members' CRC-32 and counts here
    const uint8_t* payload(const inf::Member& mb) const { return file + span_off + mb.src; }
    void crc_jobs(std::vector<crc::Job>& jobs) const
    {
        jobs.resize(members.size());
        for (size_t k = 0; k < members.size(); ++k) jobs[k] = crc::Job{members[k].dst, members[k].isize, inf::member_crc(payload(members[k]), 0, members[k].clen)};
    }
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

// the members of `r` inflated on `n_threads` host threads into dst[0, r.arena_bytes): by svt_inflate.h (`one_source`), or by the
// reader's own decoder (libdeflate / zlib); with r.verify a member that inflates has its CRC-32 checked there (inf::INF_CRC)
void inflate_round_host(const Round& r, uint8_t* dst, unsigned n_threads, bool one_source, std::vector<uint32_t>& status);

// the whole call.  0 or SVT_ERR_* with the error text set (the host scan's, when it answered).
int scan_libraries(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts, const char* const* read_groups, int64_t num_samp,
                   uint64_t round_bytes, Backend& backend, svt_library_scan* out, svt_library_scan_stats* stats);

}  // namespace lw
}  // namespace svt

#endif  // SVT_LIBRARY_ARENA_H

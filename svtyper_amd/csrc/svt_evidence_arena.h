// svt_evidence_arena.h -- what the reader (svt_reads.cpp) hands to the two callers of svt_evidence_walk.h: the arena of inflated
// BGZF payloads of one call with the per-unit record ranges in it, and the host recomputation of single units.  Internal C++
// (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_EVIDENCE_ARENA_H
#define SVT_EVIDENCE_ARENA_H

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <vector>

#include "svt_crc32.h"
#include "svt_evidence_walk.h"
#include "svt_inflate.h"

namespace svt {

// ---- verify (svt_bam_set_verify): what the handle counts, and how a call reports its share ----------------------------------------
// Whoever checks a member's CRC-32 adds to the handle's tally: the reader's threads, the arena builders, the device routes.
struct VerifyTally {
    std::atomic<uint64_t> verified{0}, failed{0}, host_ns{0}, device_ns{0};
    void add(uint64_t n_verified, uint64_t n_failed, double host_s, double device_s)
    {
        verified += n_verified;
        failed += n_failed;
        host_ns += (uint64_t)(host_s * 1e9);
        device_ns += (uint64_t)(device_s * 1e9);
    }
};
// the handle's tally when verify is on, else null: "is verify on" and "where to count" in one
VerifyTally* bam_verify(const svt_bam* bam);
// the CRC-32 of host bytes the way the reader's threads compute it: libdeflate's crc32 when its library has it, else zlib's
uint32_t host_crc32(const uint8_t* p, size_t n);
// the host-built tables of svt_crc32.h (built once), and the argument checks of svt_bgzf_crc32_host / _device
const crc::Tables& crc_tables();
int crc_check_offsets(const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint32_t* crc);
// Around a call that takes a handle: what the handle's tally gained in between becomes the calling thread's svt_bgzf_verify_stats.
// (A call inside a call -- the host scan behind a device scan -- reports into the outer one's figures: the outer scope ends last.)
struct VerifyScope {
    const svt_bam* bam;
    uint64_t verified = 0, failed = 0, host_ns = 0, device_ns = 0;
    explicit VerifyScope(const svt_bam* bam);
    ~VerifyScope();
    VerifyScope(const VerifyScope&) = delete;
    VerifyScope& operator=(const VerifyScope&) = delete;
};

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

// The arena comes from ONE planner in svt_reads.cpp with two routes.  Shared: the argument checks, the names, every unit's windows
// cut into index chunks on the reader's threads, the runs of blocks the ranges need, the 32-bit limit of the arena's offsets (a
// unit behind it is preset to EW_RANGE) and the ranges.  A route says how a chunk becomes a range and how a run is placed.

// The host route.  A chunk is inflated (the reader's block cache) and its records are walked up to the one that ends the fetch;
// a run's blocks are copied side by side.  0 or SVT_ERR_* with the error text set.
int build_arena(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out);

// ---- the arena without inflating on the host (inflate = "device") ---------------------------------------------------------------
// What build_arena_open leaves to its caller: the BGZF members whose ISIZE bytes make up the arena.  `members[k].src` is an offset
// into the compressed bytes as they are uploaded -- the file spans `spans` side by side, span k at `spans[k].at` --, `dst` the
// member's offset in the arena.  `range_members[r]`: the members arena.ranges[r] lies over (first, last).
struct OpenPlan {
    struct Span { uint64_t file_off, bytes, at; };
    const uint8_t* file = nullptr;         // the mapping of the BAM
    uint64_t file_size = 0;
    std::vector<Span> spans;
    uint64_t compressed_bytes = 0;         // sum of the spans
    uint64_t arena_bytes = 0;              // sum of the members' ISIZE
    std::vector<inf::Member> members;
    std::vector<std::pair<uint32_t, uint32_t>> range_members;
    double index_s = 0.0;
    // a member's payload in the mapping (Member.src counts in the uploaded spans: back to the file through the member's span)
    const uint8_t* payload(const inf::Member& mb) const
    {
        auto sp = std::upper_bound(spans.begin(), spans.end(), mb.src, [](uint64_t v, const Span& s) { return v < s.at; });
        --sp;
        return file + sp->file_off + (mb.src - sp->at);
    }
    // verify: the members as jobs of svt_crc32_kernel over the arena, with the CRC-32 every trailer stores
    void crc_jobs(std::vector<crc::Job>& jobs) const
    {
        jobs.resize(members.size());
        for (size_t k = 0; k < members.size(); ++k) jobs[k] = crc::Job{members[k].dst, members[k].isize, inf::member_crc(payload(members[k]), 0, members[k].clen)};
    }
};

// The open route.  A chunk is followed through BGZF headers only and becomes one range from its start to its end virtual offset
// (an upper bound; Params.open_ranges makes the walk stop where the fetch does); a run's blocks become `plan.members` out of one
// span of the file.  out.bytes is sized, not filled.
int build_arena_open(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out, OpenPlan& plan);
// the members inflated on the CPU by svt_inflate.h, straight from the mapping into out.bytes; status[k] per member.  With `verify`
// a member that inflates has its CRC-32 checked by the thread that inflated it (inf::INF_CRC).
void inflate_open_host(const OpenPlan& plan, Arena& out, unsigned n_threads, std::vector<uint32_t>& status, VerifyTally* verify = nullptr);
// every unit with a range over a member whose status is not 0 gets preset = EW_RANGE; returns the number of failed members
uint64_t apply_member_status(const OpenPlan& plan, const std::vector<uint32_t>& status, Arena& out);

// the members at block_off[] of `data` as inf::Member (dst = out_off[k]); a member that is none, or whose ISIZE is not the place
// out_off gives it, comes back with isize = inf::kNoMember
int bgzf_members(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, const uint64_t* out_off, inf::Member* members);

// the units `ids` (ascending) recomputed by the host reader: their records side by side in `records`, `counts[k]` of them for
// ids[k], `skipped[k]`.  An error is the one svt_bam_evidence reports for that unit (code returned, text set).
int host_units(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const std::vector<uint64_t>& ids,
               std::vector<svt_record>& records, std::vector<uint64_t>& counts, std::vector<uint8_t>& skipped);

}  // namespace ew
}  // namespace svt

#endif  // SVT_EVIDENCE_ARENA_H

// svt_bgzf.h -- BGZF members on the host, for both translation units of the library: the set of members every arena route
// inflates (the open-range arena, the library scan's rounds, the parity entries), the ONE host loop that inflates and verifies
// such a set, and what verify (svt_bam_set_verify) counts.  A member's header is parsed in one place, inf::member_at
// (svt_inflate.h).  Defined in svt_bgzf_reader.h, the first part of svt_reads.cpp, in front of the reader itself (svt_reads_*.h); the device side of a set is
// svt_entry_inflate.h.  Internal C++ (not exported: svt_exports.map lets only svt_* C names out).
#ifndef SVT_BGZF_H
#define SVT_BGZF_H

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <vector>

#include "../../include/svtyper_reads.h"
#include "svt_crc32.h"
#include "svt_deflate.h"
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
// the argument checks of svt_bgzf_deflate_host / _device (svt_deflate.h); `slots`: the bytes all members take at the most
int deflate_check_args(const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint8_t* out, const uint64_t* out_off, uint64_t& slots);
// What svt_huffman_lengths_host and _device refuse alike: what dfl::code_lengths asks of its histograms.
int huffman_check_args(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, const uint8_t* lengths);
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

namespace bgzf {

// Members of a mapped file, uploaded as spans side by side, inflating to an arena.  `members[k].src` is an offset into the
// compressed bytes as they are uploaded -- the file spans `spans` side by side, span k at `spans[k].at` --, `dst` the member's
// offset in the arena.  A member with isize = inf::kNoMember is none (the parity entries): it answers inf::INF_MEMBER.
struct MemberSet {
    struct Span { uint64_t file_off, bytes, at; };
    const uint8_t* file = nullptr;         // the mapping of the BAM
    uint64_t file_size = 0;
    std::vector<Span> spans;
    std::vector<inf::Member> members;
    uint64_t compressed_bytes = 0;         // sum of the spans
    uint64_t arena_bytes = 0;              // where the last member's ISIZE bytes end
    // a member's payload in the mapping (Member.src counts in the uploaded spans: back to the file through the member's span)
    const uint8_t* payload(const inf::Member& mb) const
    {
        if (spans.size() == 1) return file + spans[0].file_off + (mb.src - spans[0].at);
        auto sp = std::upper_bound(spans.begin(), spans.end(), mb.src, [](uint64_t v, const Span& s) { return v < s.at; });
        --sp;
        return file + sp->file_off + (mb.src - sp->at);
    }
    // the CRC-32 the member's trailer stores
    uint32_t stored_crc(const inf::Member& mb) const { return inf::member_crc(payload(mb), 0, mb.clen); }
    // verify: the members as jobs of svt_crc32_kernel over the arena, with the CRC-32 every trailer stores
    void crc_jobs(std::vector<crc::Job>& jobs) const
    {
        jobs.resize(members.size());
        for (size_t k = 0; k < members.size(); ++k) {
            const inf::Member& mb = members[k];            // (a member that is none fails in the inflate kernel: its job is not looked at)
            jobs[k] = mb.isize == inf::kNoMember ? crc::Job{0, 0, 0} : crc::Job{mb.dst, mb.isize, stored_crc(mb)};
        }
    }
};

// The arguments of svt_bgzf_inflate_host / _device checked, and the members at block_off[] of `data` as one span (dst =
// out_off[k]); a member that is none, or whose ISIZE is not the place out_off gives it, comes back with isize = inf::kNoMember.
int bgzf_members(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, const uint8_t* out, const uint64_t* out_off,
                 const uint32_t* status, MemberSet& set);

// who inflates a member on the host: svt_inflate.h as the kernel runs it (inf::inflate_member<HostCtx>), or the reader's library
// decoder (libdeflate, else zlib); and who computes its CRC-32: host_crc32, or svt_crc32.h as the kernel runs it
enum class Decoder { one_source, library };
enum class Crc { library, one_source };

// The members of `set` inflated on `n_threads` host threads (batches of 8 from one counter) straight from the mapping into
// dst[0, set.arena_bytes); status[k] = inf::INF_* per member.  With `verify` a member that inflates has its CRC-32 checked by
// the thread that inflated it (inf::INF_CRC) and is counted there.
void inflate_members_host(const MemberSet& set, uint8_t* dst, unsigned n_threads, Decoder decoder, Crc crc, VerifyTally* verify,
                          std::vector<uint32_t>& status);

}  // namespace bgzf
}  // namespace svt

#endif  // SVT_BGZF_H

// svt_reads.cpp -- native BAM access + fragment summariser (include/svtyper_reads.h).
//
// Host-only C++ (no HIP): BAM/BAI reader over the BGZF layer of svt_bgzf_reader.h, with the fetch()/count() semantics the SVTyper path
// relies on (pysam's, as restated in svtyper_amd/bam.py), read-fragment assembly and split-read QC
// (svtyper/parsers.py:729-768, 891-1058 as restated in svtyper_amd/fragments.py) and the emission of
// svt_fragment summaries (svtyper_amd/geometry.py).  The Python modules are the portable
// implementation and the checker of this file (tests/test_native_reads.py compares the summaries
// byte for byte); this file exists because per-read Python objects, not the GPU, bound a real run.

#include <sys/mman.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/svtyper_reads.h"
#include "svt_bam_index.h"
#include "svt_bgzf.h"
#include "svt_dump_rules.h"
#include "svt_error.h"
#include "svt_evidence_arena.h"
#include "svt_geometry_math.h"
#include "svt_host_cpus.h"
#include "svt_library_arena.h"
#include "svt_record_rules.h"

#include "svt_bgzf_reader.h"   // FileMap, Bgzf and the host loop over a bgzf::MemberSet: this translation unit's BGZF layer

namespace {

using svt::fail;
using svt::guarded;
using svt::run_threads;
namespace rr = svt::rr;

std::atomic<double> g_cpu_s_per_unit{0.0};   // CPU seconds per unit of the last svt_bam_summarise / svt_bam_evidence call on any file

// ------------------------------------------------------------------------------------------
// reads, pieces, fragments (what a record means is svt_record_rules.h)
// ------------------------------------------------------------------------------------------
struct ReadInfo {                // what a primary read contributes to a summary (svt_read_summary)
    int32_t tid = -1;
    int64_t start = 0, end = 0;
    bool reverse = false;
    int mapq = 0;
    int n_iv = 0;                // the (at most two) gap-free aligned intervals closest to the unit's breakends
    int64_t iv_start[2] = {0, 0}, iv_end[2] = {0, 0};
};

struct PieceOut {                // what a split piece contributes to a summary (svt_piece_summary)
    int32_t tid = 0;
    int64_t start = 0, end = 0, mapq = 0;
    bool reverse = false;
};

struct SplitOut {
    bool soft = false;
    PieceOut left, right;
};

struct Fragment {                // reused from unit to unit (its vectors keep their capacity)
    int lib = 0;
    int num_primary = 0;
    uint32_t name_off = 0, name_len = 0;   // query name in the workspace's name arena
    std::vector<uint16_t> seen;            // flags already added under this query name (parsers.py:748-754)
    std::vector<ReadInfo> primaries;
    std::vector<SplitOut> splits;
    void reset(int library, uint32_t off, uint32_t len)
    {
        lib = library;
        num_primary = 0;
        name_off = off;
        name_len = len;
        seen.clear();
        primaries.clear();
        splits.clear();
    }
};

// One BAM alignment: the fixed fields (rr::Core) and the record's bytes -- inside the inflated block, or the caller's gather
// buffer for a record that straddles blocks: valid until the next record is read.
struct Record : rr::Core {
    const uint8_t* data = nullptr;
    uint32_t size = 0;
    const char* name() const { return reinterpret_cast<const char*>(data + 32); }
    uint32_t name_len() const { return l_name ? l_name - 1 : 0; }
    const uint8_t* cigar() const { return data + 32 + l_name; }     // n_cigar words
    int64_t tlen() const { return (int32_t)rr::ld32(data + 28); }   // template_length
    std::string name_str() const { return std::string(name(), name_len()); }
};

// The first leg of a kept read's tag walk (svtyper_amd/bam.py::_parse_tags): up to its RG value, noting an SA value met on the
// way.  nullptr: no usable RG tag.  A read that becomes a split candidate walks on from `at` (tags_behind_rg); every other
// kept read stops here.  A value that runs over the record's end ends the walk without a complaint (rr::TAGS_OVERRUN).
const char* read_group(const Record& r, rr::Tags& t, uint32_t& at)
{
    rr::tags_begin(t);
    at = r.tags_off;
    if (rr::walk_tags(r.data, r.size, at, /*stop_at_rg=*/true, t) != rr::TAGS_AT_RG) return nullptr;
    return reinterpret_cast<const char*>(r.data + t.rg_off);
}
// The second leg: every tag behind RG is validated (a malformed tag anywhere fails the call, as bam.py raises:
// tests/test_native_reads.py::test_truncated_tag_behind_rg_is_malformed_in_both_tag_orders) and the first SA value noted.
bool tags_behind_rg(const Record& r, rr::Tags& t, uint32_t at)
{
    return rr::walk_tags(r.data, r.size, at, false, t) != rr::TAGS_MALFORMED;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// the BAM handle: header + index (shared, read-only); file handles are per thread
// ------------------------------------------------------------------------------------------
struct svt_bam {
    std::string path;
    FileMap file;
    std::string text;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lengths;
    std::unordered_map<std::string, int32_t> tid_of;
    uint64_t first_record = 0;
    svt::bamidx::Index index;      // BAI or CSI behind one model (svt_bam_index.h); kind KIND_NONE: the file has none
    bool has_index() const { return index.kind != svt::bamidx::KIND_NONE; }
    // CPU seconds per unit of the summariser's last calls on this file (0: none yet): sizes the next call's burst
    mutable std::atomic<double> cpu_s_per_unit{0.0};
    // svt_bam_set_verify: off by default; the tally of everything that was verified through this handle
    std::atomic<int> verify{0};
    mutable svt::VerifyTally tally;
};

static thread_local svt_bgzf_verify_counts g_verify_stats{};   // svt_bgzf_verify_stats: this thread's last call that took a handle

namespace svt {

VerifyTally* bam_verify(const svt_bam* bam) { return bam && bam->verify.load() ? &bam->tally : nullptr; }

VerifyScope::VerifyScope(const svt_bam* b) : bam(b)
{
    g_verify_stats = svt_bgzf_verify_counts{};
    if (!bam) return;
    verified = bam->tally.verified.load();
    failed = bam->tally.failed.load();
    host_ns = bam->tally.host_ns.load();
    device_ns = bam->tally.device_ns.load();
}
VerifyScope::~VerifyScope()
{
    if (!bam) return;
    g_verify_stats.members_verified = bam->tally.verified.load() - verified;
    g_verify_stats.members_failed = bam->tally.failed.load() - failed;
    g_verify_stats.host_crc_s = (double)(bam->tally.host_ns.load() - host_ns) * 1e-9;
    g_verify_stats.device_crc_s = (double)(bam->tally.device_ns.load() - device_ns) * 1e-9;
}

}  // namespace svt

namespace {

using rr::ld32;

// The bytes of the next alignment (after its length word): in place inside the inflated block when the
// record does not straddle a block boundary -- no copy, which is what makes walking up to a window cheap
// -- otherwise gathered into `buf`.  nullptr at the end of the data / on a bad length.
const uint8_t* next_record(Bgzf& z, std::vector<uint8_t>& buf, uint32_t& size)
{
    constexpr uint32_t kMaxRecord = 1u << 28;   // no alignment record is a quarter of a gigabyte: a corrupt length
    if (const uint8_t* h = z.contiguous(4)) {
        size = ld32(h);
        if (size < 32 || size > kMaxRecord) { z.mark_bad(); return nullptr; }
        if (const uint8_t* d = z.contiguous(4 + (size_t)size)) {
            z.advance(4 + (size_t)size);
            return d + 4;
        }
    }
    uint8_t szb[4];
    if (z.read(szb, 4) != 4) return nullptr;
    size = ld32(szb);
    if (size < 32 || size > kMaxRecord) { z.mark_bad(); return nullptr; }
    buf.resize(size);
    if (z.read(buf.data(), size) != size) return nullptr;
    return buf.data();
}

// fixed fields + reference end: all a fetch needs to decide whether the record overlaps its window
bool decode(const uint8_t* d, uint32_t size, Record& r)
{
    r.data = d;
    r.size = size;
    return d && rr::decode_core(d, size, r);
}

bool read_record(Bgzf& z, std::vector<uint8_t>& buf, Record& r)
{
    uint32_t size = 0;
    const uint8_t* d = next_record(z, buf, size);
    return decode(d, size, r);
}

// the merged index chunks a fetch of [beg, end) on `tid` walks, in file order (scratch of the calling thread)
const std::vector<std::pair<uint64_t, uint64_t>>& fetch_chunks(const svt_bam& bam, int32_t tid, int64_t beg, int64_t end)
{
    // (reused from fetch to fetch: two fetches per unit, three allocations each)
    static thread_local std::vector<uint32_t> bins;
    static thread_local std::vector<std::pair<uint64_t, uint64_t>> chunks, merged;
    bam.index.fetch_chunks(tid, beg, end, bam.ref_lengths[tid], bins, chunks, merged);
    return merged;
}

// pysam-style fetch: records with pos < end and reference end > beg, in file order; `fn` returns
// false to stop.  Mirrors svtyper_amd/bam.py::AlignmentFile.fetch.
template <typename Fn>
bool fetch(const svt_bam& bam, Bgzf& z, int32_t tid, int64_t beg, int64_t end, std::vector<uint8_t>& buf, Fn&& fn)
{
    if (tid < 0 || tid >= (int32_t)bam.ref_names.size()) return false;
    beg = std::max<int64_t>(beg, 0);
    if (end <= beg) return true;
    const auto& merged = fetch_chunks(bam, tid, beg, end);
    if (merged.empty()) return true;
    Record r;
    for (const auto& c : merged) {
        z.seek(c.first);
        while (z.tell() < c.second) {
            uint32_t size = 0;
            const uint8_t* d = next_record(z, buf, size);
            if (!decode(d, size, r)) break;
            // (verify: a fetch that ends early has still read through a block whose CRC-32 did not match)
            if (r.tid != tid || r.pos >= end) return !z.crc_failed();
            int64_t rend = r.end;
            if (r.n_cigar == 0 || rend <= r.pos) rend = (int64_t)r.pos + 1;
            if (rend > beg && !fn(r)) return !z.crc_failed();      // (most records walked on the way to the window stop here)
        }
    }
    return !z.failed();
}

// SplitRead.is_valid (parsers.py:959-1058 / fragments.py) -> fills `out` when the candidate is valid
// returns 1 valid, 0 invalid, -1 malformed input.  The rules are rr::; the host reader's own: an SA number is what strtoll
// reads over the whole field, a chromosome name goes through the header's map, and there is no limit on lengths.
int split_candidate(const svt_bam& bam, const Record& r, const rr::Tags& t, SplitOut& out)
{
    if (r.n_cigar == 0) return 0;   // a mapped read without a CIGAR cannot be a split candidate (fragments.py: add_read)
    rr::CigarStats a;
    rr::cigar_of_words(r.cigar(), r.n_cigar, a);
    const bool a_rev = (r.flag & 0x10) != 0;
    const PieceOut self{r.tid, r.pos, r.end, (int64_t)r.mapq, a_rev};
    bool self_left;
    PieceOut other;
    if (!t.have_sa) {
        if (!rr::soft_clip_candidate(a, r.l_seq)) return 0;
        other = PieceOut{-2, 1, 1, 0, a_rev};           // the dummy piece (chrom None)
        self_left = !rr::left_clipped(a);
    } else {
        const uint8_t* sa = r.data + t.sa_off;
        uint32_t fo[5], fl[5];
        uint32_t entries;
        const uint32_t fields = rr::sa_fields(sa, t.sa_len, entries, fo, fl);
        if (entries > 1) return 0;                      // more than one entry -> discarded (:992-993)
        if (fields < 5) return -1;
        auto whole_number = [&](int k, long long& v) {  // strtoll over the whole field
            char buf[32];
            if (fl[k] == 0 || fl[k] >= sizeof buf) return false;
            std::memcpy(buf, sa + fo[k], fl[k]);
            buf[fl[k]] = 0;
            char* endp = nullptr;
            v = std::strtoll(buf, &endp, 10);
            return *endp == 0;
        };
        long long mate_pos1 = 0, mate_mapq = 0;
        rr::CigarStats b;
        if (!whole_number(1, mate_pos1) || !whole_number(4, mate_mapq)) return -1;
        if (rr::cigar_of_string(sa + fo[3], fl[3], UINT32_MAX, 18, b) != rr::CIGAR_OK) return -1;
        const std::string sa_chrom(reinterpret_cast<const char*>(sa) + fo[0], fl[0]);    // (chromosome names fit the small-string buffer)
        auto it = bam.tid_of.find(sa_chrom);
        const bool b_rev = fl[2] == 1 && sa[fo[2]] == '-';
        other = PieceOut{it == bam.tid_of.end() ? -3 : it->second, mate_pos1 - 1, mate_pos1 - 1 + b.ref, mate_mapq, b_rev};
        const rr::Piece pa = {self.tid, self.start, self.end, a_rev, rr::query_pos(a, a_rev)};
        const rr::Piece pb = {other.tid, other.start, other.end, b_rev, rr::query_pos(b, b_rev)};
        const bool same_chrom = r.tid >= 0 && bam.ref_names[r.tid] == sa_chrom;
        if (!rr::split_valid(pa, pb, same_chrom, rr::left_clipped(a), self_left)) return 0;
    }
    out.soft = !t.have_sa;
    out.left = self_left ? self : other;
    out.right = self_left ? other : self;
    return 1;
}

using rr::clip32;

void fill_read(svt_read_summary& d, const ReadInfo& r)
{
    d.tid = r.tid;
    d.start = clip32(r.start);
    d.end = clip32(r.end);
    for (int k = 0; k < r.n_iv; ++k) {
        d.iv_start[k] = clip32(r.iv_start[k]);
        d.iv_end[k] = clip32(r.iv_end[k]);
    }
    d.mapq = (uint8_t)r.mapq;
    d.flags = (uint8_t)(SVT_READ_PRESENT | (r.reverse ? SVT_READ_REVERSE : 0));
}

bool fill_piece(svt_piece_summary& d, const PieceOut& p)
{
    if (p.mapq < 0) return false;
    d.tid = p.tid;
    d.start = clip32(p.start);
    d.end = clip32(p.end);
    d.mapq = (uint8_t)std::min<int64_t>(p.mapq, 255);   // an SA-tag MAPQ above 255: prob_mapq is exactly 1.0 from 163 on (packer.py: _mapq)
    d.flags = (uint8_t)(SVT_READ_PRESENT | (p.reverse ? SVT_READ_REVERSE : 0));
    return true;
}

struct UnitOut {                       // per worker, reused for every unit it processes
    std::vector<svt_fragment> frags;
    std::vector<svt_record> recs;      // svt_bam_evidence: the summaries turned into evidence records
    bool skipped = false;
};

// Per-worker scratch of process_unit, reused from unit to unit so that a read costs no allocation: the
// read-fragments of the unit (query name -> Fragment) live in a vector indexed through an open-addressing
// hash table over a name arena, and are emitted in sorted(query_name) order at the end.
struct Workspace {
    std::vector<Fragment> frags;       // [0, n_frags) are live
    size_t n_frags = 0;
    std::vector<char> names;
    std::vector<uint64_t> table;       // (name hash's high half) << 32 | fragment index + 1, 0 = empty; size is a power of two
    std::vector<uint32_t> order;
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    std::vector<uint64_t> packed;
    std::vector<const SplitOut*> seq, clip;
    std::string last_rg;               // most reads of a unit share their read group
    int32_t last_lib = 0;
    bool have_last_rg = false;

    void begin_unit()
    {
        n_frags = 0;
        names.clear();
        if (table.size() < 1024) table.assign(1024, 0ull);
        else std::fill(table.begin(), table.end(), 0ull);
    }
    static uint64_t hash_name(const char* p, size_t n)
    {
        // eight bytes per step: a byte-wise FNV-1a is a serial chain of one multiply per byte of a 20-50 byte name (a tenth of
        // what a kept read costs)
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        size_t i = 0;
        for (; i + 8 <= n; i += 8) {
            uint64_t w;
            std::memcpy(&w, p + i, 8);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        if (i < n) {
            uint64_t w = 0;
            std::memcpy(&w, p + i, n - i);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        return h;
    }
    const char* name_of(const Fragment& f) const { return names.data() + f.name_off; }
    // the fragment of this query name; created (with `lib`) when the name is new
    Fragment& fragment(const char* name, const uint32_t len, int lib)
    {
        if ((n_frags + 1) * 2 > table.size()) grow();
        const size_t mask = table.size() - 1;
        const uint64_t h = hash_name(name, len), tag = h & 0xffffffff00000000ull;
        // the slot carries the hash's high half: a probe that meets another name's slot moves on without touching that
        // fragment (a big struct) or its name; the second read of a pair pays ONE memcmp
        for (size_t i = h & mask;; i = (i + 1) & mask) {
            const uint64_t e = table[i];
            if (e == 0ull) {
                if (n_frags == frags.size()) frags.emplace_back();
                Fragment& f = frags[n_frags];
                f.reset(lib, (uint32_t)names.size(), len);
                names.insert(names.end(), name, name + len);
                table[i] = tag | (uint64_t)++n_frags;
                return f;
            }
            if ((e & 0xffffffff00000000ull) != tag) continue;
            Fragment& f = frags[(uint32_t)e - 1];
            if (f.name_len == len && std::memcmp(name_of(f), name, len) == 0) return f;
        }
    }
    void grow()
    {
        table.assign(table.size() * 2, 0ull);
        const size_t mask = table.size() - 1;
        for (size_t k = 0; k < n_frags; ++k) {
            const uint64_t h = hash_name(name_of(frags[k]), frags[k].name_len);
            size_t i = h & mask;
            while (table[i]) i = (i + 1) & mask;
            table[i] = (h & 0xffffffff00000000ull) | (uint64_t)(k + 1);
        }
    }
    // live fragments in the order of Python's sorted() over their (ASCII) names.  Query names of one run share a long
    // prefix (instrument : run : flowcell : lane ...), so comparing them byte by byte from the start -- a few hundred
    // times per unit -- reads the same thirty bytes again and again: the common prefix of the unit's names is found once
    // and the sort runs on the eight bytes behind it as one big-endian integer; equal keys fall back to the whole names.
    const std::vector<uint32_t>& sorted_order()
    {
        order.resize(n_frags);
        keys.resize(n_frags);
        size_t lcp = n_frags ? frags[0].name_len : 0;
        for (size_t k = 1; k < n_frags && lcp; ++k) {
            const char *a = name_of(frags[0]), *b = name_of(frags[k]);
            const size_t n = std::min<size_t>(lcp, frags[k].name_len);
            size_t i = 0;
            for (; i + 8 <= n; i += 8) {      // eight bytes at a time: thirty common bytes times a few hundred names per unit
                uint64_t x, y;
                std::memcpy(&x, a + i, 8);
                std::memcpy(&y, b + i, 8);
                if (x != y) { i += (size_t)__builtin_ctzll(x ^ y) >> 3; break; }     // (little-endian: the lowest differing byte)
            }
            while (i < n && a[i] == b[i]) ++i;      // (the tail; at once over when the words differed)
            lcp = i;
        }
        auto key_of = [&](const Fragment& f) {
            uint64_t key = 0;                                    // bytes past the end count as 0: a shorter name sorts first,
            const unsigned char* p = reinterpret_cast<const unsigned char*>(name_of(f)) + lcp;   // as it does for memcmp + length
            const size_t have = f.name_len - lcp;               // (lcp <= every name's length)
            if (have >= 8) {
                std::memcpy(&key, p, 8);
                return __builtin_bswap64(key);
            }
            for (size_t i = 0; i < 8; ++i) key = (key << 8) | (i < have ? p[i] : 0u);
            return key;
        };
        auto by_name = [&](const uint32_t x, const uint32_t y) {
            const Fragment &a = frags[x], &b = frags[y];
            const int c = std::memcmp(name_of(a), name_of(b), std::min(a.name_len, b.name_len));
            return c != 0 ? c < 0 : a.name_len < b.name_len;
        };
        if (n_frags <= 4096) {
            // the usual unit: the key's leading 52 bits and the fragment's index in ONE integer -- a sort of plain 64-bit words, no
            // comparator that looks at the names; runs of equal leading bits (rare: they agree in six and a half bytes behind the
            // common prefix) are put in order by their whole names afterwards
            packed.resize(n_frags);
            for (size_t k = 0; k < n_frags; ++k) packed[k] = (key_of(frags[k]) & ~uint64_t(0xfff)) | (uint64_t)k;
            std::sort(packed.begin(), packed.end());
            for (size_t k = 0; k < n_frags; ++k) order[k] = (uint32_t)(packed[k] & 0xfffu);
            for (size_t k = 0; k < n_frags;) {
                size_t e = k + 1;
                while (e < n_frags && (packed[e] >> 12) == (packed[k] >> 12)) ++e;
                if (e - k > 1) std::sort(order.begin() + (ptrdiff_t)k, order.begin() + (ptrdiff_t)e, by_name);
                k = e;
            }
            return order;
        }
        for (size_t k = 0; k < n_frags; ++k) keys[k] = std::make_pair(key_of(frags[k]), (uint32_t)k);
        std::sort(keys.begin(), keys.end(), [&](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) {
            if (x.first != y.first) return x.first < y.first;
            return by_name(x.second, y.second);
        });
        for (size_t k = 0; k < n_frags; ++k) order[k] = keys[k].second;
        return order;
    }
};

struct UnitSpan {                      // where a finished unit's summaries (or evidence records) wait for the gather
    const void* data = nullptr;
    uint64_t count = 0;
    bool skipped = false;
};

// Large host buffers of the summariser (the workers' arenas, the flat summary array): anonymous mappings advised for
// transparent huge pages -- the summaries are written once and read once, so what they cost is page faults and, when they
// go, the unmapping: on the 2 x EPYC 9575F box 17 ms to unmap the arenas of 2.1 M summaries and as much again for the
// flat array, a third of the call.  Mappings therefore go back to a process-wide pool (at most SVT_READER_POOL_MB, default
// 1024, of idle memory; 0 = unmap at once) and the next call starts on pages that are already there.
class BufferPool {
public:
    static BufferPool& get()
    {
        static BufferPool* pool = new BufferPool();      // (never destroyed: buffers may be returned during process exit)
        return *pool;
    }
    // a mapping of at least `bytes` (its real size goes to *cap), nullptr when the system has none
    void* acquire(size_t bytes, size_t* cap)
    {
        const size_t want = (std::max<size_t>(bytes, 1) + kGrain - 1) / kGrain * kGrain;
        {
            std::lock_guard<std::mutex> g(lock_);
            size_t best = idle_.size();
            for (size_t i = 0; i < idle_.size(); ++i)    // smallest idle mapping that fits and is not more than twice too big
                if (idle_[i].second >= want && idle_[i].second <= 2 * want && (best == idle_.size() || idle_[i].second < idle_[best].second)) best = i;
            if (best != idle_.size()) {
                void* p = idle_[best].first;
                *cap = idle_[best].second;
                idle_bytes_ -= *cap;
                idle_.erase(idle_.begin() + (long)best);
                return p;
            }
        }
        void* p = mmap(nullptr, want, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return nullptr;
        madvise(p, want, MADV_HUGEPAGE);
        *cap = want;
        return p;
    }
    void release(void* p, size_t cap)
    {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(lock_);
            if (idle_bytes_ + cap <= limit_) {
                idle_.emplace_back(p, cap);
                idle_bytes_ += cap;
                return;
            }
        }
        munmap(p, cap);
    }
    // the flat array handed to the caller: its size is remembered here so that svt_summaries_free needs only the pointer
    void* acquire_tracked(size_t bytes)
    {
        size_t cap = 0;
        void* p = acquire(bytes, &cap);
        if (p) {
            std::lock_guard<std::mutex> g(lock_);
            lent_[p] = cap;
        }
        return p;
    }
    // unmap every idle mapping (svt_trim): a long-lived embedding process gives the pool's memory back
    void trim()
    {
        std::vector<std::pair<void*, size_t>> idle;
        {
            std::lock_guard<std::mutex> g(lock_);
            idle.swap(idle_);
            idle_bytes_ = 0;
        }
        for (const auto& m : idle) munmap(m.first, m.second);
    }
    bool release_tracked(void* p)
    {
        size_t cap = 0;
        {
            std::lock_guard<std::mutex> g(lock_);
            auto it = lent_.find(p);
            if (it == lent_.end()) return false;
            cap = it->second;
            lent_.erase(it);
        }
        release(p, cap);
        return true;
    }

private:
    BufferPool()
    {
        if (const char* e = std::getenv("SVT_READER_POOL_MB")) limit_ = (size_t)std::max(0ll, std::atoll(e)) << 20;
    }
    static constexpr size_t kGrain = 2u << 20;           // one huge page
    std::mutex lock_;
    std::vector<std::pair<void*, size_t>> idle_;
    std::unordered_map<void*, size_t> lent_;
    size_t idle_bytes_ = 0, limit_ = (size_t)1024 << 20;
};

// append-only store of one worker: units are copied in whole, never split across chunks
class SummaryArena {
public:
    SummaryArena() = default;
    SummaryArena(const SummaryArena&) = delete;
    SummaryArena& operator=(const SummaryArena&) = delete;
    ~SummaryArena() { for (auto& c : chunks_) BufferPool::get().release(c.first, c.second); }
    const void* append(const void* data, size_t bytes)
    {
        if (bytes == 0) return nullptr;
        if (used_ + bytes > cap_) {
            size_t size = 0;     // 2, 4, 8, 16, 16 ... MiB: forty-seven workers of a small call do not map (and return) 16 MiB each
            void* p = BufferPool::get().acquire(std::max(bytes, std::min(kChunkBytes, (size_t)(2u << 20) << std::min<size_t>(chunks_.size(), 3))), &size);
            if (!p) return nullptr;
            chunks_.emplace_back(p, size);
            cap_ = size;
            used_ = 0;
        }
        uint8_t* dst = static_cast<uint8_t*>(chunks_.back().first) + used_;
        std::memcpy(dst, data, bytes);
        used_ += bytes;
        return dst;
    }

private:
    static constexpr size_t kChunkBytes = 16u << 20;
    std::vector<std::pair<void*, size_t>> chunks_;
    size_t cap_ = 0, used_ = 0;
};

inline double thread_cpu_seconds()
{
    timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec : 0.0;
}

// one unit: gather reads of both windows, assemble fragments, emit summaries
// `emit(fragment)`: what becomes of a finished summary -- kept as it is (svt_bam_summarise) or turned into its 16-byte evidence
// record on the spot (svt_bam_evidence: no array of 128-byte summaries in between); returns false with `err` set to stop
template <typename Emit>
int process_unit(const svt_bam& bam, Bgzf& z, std::vector<uint8_t>& buf, const svt_summarise_args& A,
                 const std::unordered_map<std::string, int32_t>& rg_lib, uint64_t u, Workspace& ws, UnitOut& out,
                 std::string& err, Emit&& emit)
{
    out.frags.clear();
    out.recs.clear();
    out.skipped = false;
    const svt_fetch_unit& w = A.windows[u];
    const int32_t tids[2] = {w.tid_a, w.tid_b};
    const int64_t los[2] = {w.lo_a, w.lo_b}, his[2] = {w.hi_a, w.hi_b};
    const int64_t near_a = A.breakpoints[u].pos_a, near_b = A.breakpoints[u].pos_b;
    ws.begin_unit();
    int rc = SVT_OK;

    // count_mode 1 (singlesample.py:158-185): a unit is skipped when bam.count() of either window exceeds
    // max_reads.  count() looks at the same records the gather pass walks, so the two are one pass here: the
    // reads of a window are counted (pysam's filter: not unmapped / secondary / QC-fail / duplicate) while
    // they are gathered, and the unit is dropped when a window turns out to be over the limit.
    const bool count_windows = A.count_mode == 1 && A.max_reads >= 0;
    for (int s = 0; s < 2 && !out.skipped; ++s) {
        int64_t i = -1, n_counted = 0;
        const bool ok = fetch(bam, z, tids[s], los[s], his[s], buf, [&](const Record& r) {
            ++i;                                                        // enumerate() index of classic.py:79
            if (count_windows && !(r.flag & (0x4 | 0x100 | 0x200 | 0x400)) && ++n_counted > A.max_reads) {
                out.skipped = true;
                return false;
            }
            if (r.flag & (0x4 | 0x400)) return true;                   // unmapped / duplicate
            rr::Tags tags;
            uint32_t behind_rg = 0;
            const char* rg = read_group(r, tags, behind_rg);
            if (!rg) { err = "read without a usable RG tag: " + r.name_str(); rc = SVT_ERR_INVALID; return false; }
            if (!ws.have_last_rg || ws.last_rg != rg) {
                auto it = rg_lib.find(rg);
                if (it == rg_lib.end()) { err = std::string("read group not in the library table: ") + rg; rc = SVT_ERR_INVALID; return false; }
                ws.last_rg = rg;
                ws.last_lib = it->second;
                ws.have_last_rg = true;
            }
            if (ws.last_lib < 0) return true;                           // library below the prevalence cut
            if (A.count_mode == 0 && A.max_reads >= 0 && i > A.max_reads) { out.skipped = true; return false; }
            Fragment& f = ws.fragment(r.name(), r.name_len(), ws.last_lib);             // SamFragment(read, lib) when new
            if (std::find(f.seen.begin(), f.seen.end(), r.flag) != f.seen.end()) return true;   // same (name, flag) again
            f.seen.push_back(r.flag);
            if (r.flag & (0x100 | 0x800)) return true;                  // secondary / supplementary
            ReadInfo ri;
            ri.tid = r.tid;
            ri.start = r.pos;
            ri.end = r.end;
            ri.reverse = (r.flag & 0x10) != 0;
            ri.mapq = (int)r.mapq;
            rr::Intervals iv;
            rr::aligned_intervals(r.cigar(), r.n_cigar, r.pos, near_a, near_b, iv);
            ri.n_iv = (int)iv.n;
            for (int k = 0; k < 2; ++k) { ri.iv_start[k] = iv.s[k]; ri.iv_end[k] = iv.e[k]; }
            f.primaries.push_back(ri);
            f.num_primary += 1;
            SplitOut sp;
            const int v = tags_behind_rg(r, tags, behind_rg) ? split_candidate(bam, r, tags, sp) : -1;
            if (v < 0) { err = "malformed SA tag / CIGAR at read " + r.name_str(); rc = SVT_ERR_INVALID; return false; }
            if (v > 0) f.splits.push_back(sp);
            return true;
        });
        if (rc != SVT_OK) return rc;
        if (!ok) { err = z.crc_failed() ? z.crc_error() : "BAM read error"; return SVT_ERR_INVALID; }
    }
    if (out.skipped) { out.frags.clear(); out.recs.clear(); return SVT_OK; }

    for (const uint32_t fi : ws.sorted_order()) {
        const Fragment& f = ws.frags[fi];
        ws.seq.clear();
        ws.clip.clear();
        for (const SplitOut& sp : f.splits) (sp.soft ? ws.clip : ws.seq).push_back(&sp);
        const size_t n_rec = std::max<size_t>({(size_t)1, (f.primaries.size() + 1) / 2, ws.seq.size(), ws.clip.size()});
        for (size_t k = 0; k < n_rec; ++k) {
            svt_fragment fr;
            std::memset(&fr, 0, sizeof fr);
            fr.read[0].tid = fr.read[1].tid = -1;
            for (int j = 0; j < 2; ++j)
                if (2 * k + j < f.primaries.size()) fill_read(fr.read[j], f.primaries[2 * k + j]);
            fr.read[0].reserved = (uint16_t)f.lib;
            fr.read[1].reserved = (uint16_t)(((k == 0 && f.num_primary == 2) ? SVT_FRAG_PAIR : 0) | (k > 0 ? SVT_FRAG_CONTINUATION : 0));
            bool ok = true;
            if (k < ws.seq.size()) ok = fill_piece(fr.seq[0], ws.seq[k]->left) && fill_piece(fr.seq[1], ws.seq[k]->right);
            if (ok && k < ws.clip.size()) ok = fill_piece(fr.clip[0], ws.clip[k]->left) && fill_piece(fr.clip[1], ws.clip[k]->right);
            if (!ok) {
                err = "MAPQ outside 0..255 in an SA tag of fragment " + std::string(ws.name_of(f), f.name_len);
                return SVT_ERR_INVALID;
            }
            if (!emit(fr)) return SVT_ERR_INVALID;
        }
    }
    return SVT_OK;
}

// one unit as evidence records (unit.recs): process_unit with the predicates of the device stage as its emitter
int evidence_unit(const svt_bam& bam, Bgzf& z, std::vector<uint8_t>& buf, const svt_summarise_args& A, const svt_evidence_params& G,
                  const std::unordered_map<std::string, int32_t>& rg_lib, uint64_t u, Workspace& ws, UnitOut& unit, std::string& err)
{
    const svt_breakpoint& bp = A.breakpoints[u];
    if (bp.svtype > SVT_SVTYPE_BND) { err = "bad svtype"; return SVT_ERR_INVALID; }
    return process_unit(bam, z, buf, A, rg_lib, u, ws, unit, err, [&](const svt_fragment& f) {
        const uint32_t lib = f.read[0].reserved;
        if (lib >= G.n_libs) { err = "library index of a fragment outside the library table"; return false; }
        const svt::Record4 r = svt::geometry_record(svt::read_of(f.read[0]), svt::read_of(f.read[1]), svt::piece_of(f.seq[0]),
                                                    svt::piece_of(f.seq[1]), svt::piece_of(f.clip[0]), svt::piece_of(f.clip[1]), bp,
                                                    G.lib_flank[lib], G.min_aligned, G.split_slop);
        static_assert(sizeof(svt_record) == sizeof r, "svt_record is four words");
        unit.recs.emplace_back();
        std::memcpy(&unit.recs.back(), &r, sizeof r);
        return true;
    });
}

}  // namespace

// ------------------------------------------------------------------------------------------
// the arena of svt_evidence_walk.h and the host recomputation of single units (svt_evidence_arena.h)
// ------------------------------------------------------------------------------------------
namespace svt {
namespace ew {

namespace {

unsigned arena_threads(const svt_summarise_args* args, uint64_t n)
{
    unsigned nt = args->n_threads > 0 ? (unsigned)args->n_threads : std::max(1u, svt::burst_threads((double)n * 350e-6, 48u) - 1u);
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt ? nt : 1, n ? n : 1));
}

// ---- one planner for both routes of the arena.  A route says how one index chunk becomes one range (its Worker) and how a run of
// blocks is placed (what it hands to place_runs); everything else is the code below.

// Offsets into the arena are 32 bits: the units whose ranges lie beyond 4 GiB of inflated blocks are left to the host reader
// (EW_RANGE; svt_evidence_device_stats.units_host_by_reason shows them).  On the host route the blocks stay alive until the arena
// is put together, so a call holds twice its inflated bytes for a moment: the drivers hand the reader blocks of sites
// (pipeline.CHUNK_UNITS), a few hundred MiB at 30x, far below either limit.
constexpr uint64_t kArenaLimit = 0xFFFF0000ull;

int check_arena_args(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry)
{
    if (!bam || !args || !geometry) return fail(SVT_ERR_INVALID, "null argument");
    if (geometry->n_libs == 0 || geometry->n_libs > 65536 || !geometry->lib_flank)
        return fail(SVT_ERR_INVALID, "n_libs must be 1..65536 with a flank per library");
    if (args->n_units && (!args->windows || !args->breakpoints)) return fail(SVT_ERR_INVALID, "null unit arrays");
    if (args->n_units >= 0xFFFFFFF0ull) return fail(SVT_ERR_INVALID, "too many units in one call (< 2^32)");
    return SVT_OK;
}

// the read-group ids and reference names: out.rgs, out.refs and their bytes in out.blob (8 bytes of padding behind them)
void arena_names(const svt_bam* bam, const svt_summarise_args* args, Arena& out)
{
    auto add_name = [&](std::vector<NameRef>& tab, const char* p, size_t len, int32_t value) {
        tab.push_back(NameRef{(uint32_t)out.blob.size(), (uint32_t)len, value});
        out.blob.insert(out.blob.end(), p, p + len);
    };
    for (uint32_t i = 0; i < args->n_read_groups; ++i) add_name(out.rgs, args->read_groups[i], std::strlen(args->read_groups[i]), args->read_group_lib[i]);
    for (size_t i = 0; i < bam->ref_names.size(); ++i) add_name(out.refs, bam->ref_names[i].data(), bam->ref_names[i].size(), (int32_t)i);
    out.blob.resize(out.blob.size() + 8, 0);
}

// One index chunk's records: its first block, the in-block offset of its first record, the block that holds its last byte and
// its end as an offset from that block's start.  (A run's blocks lie side by side in the arena, so the end needs no length.)
struct RawRange { uint64_t first, last; uint32_t uoff, end_in_last; };
struct UnitRaw { uint64_t at = 0; unsigned worker = 0; uint16_t n[2] = {0, 0}; uint32_t preset = EW_OK; };   // at: in its worker's list
struct UnitPlan { std::vector<UnitRaw> units; std::vector<std::vector<RawRange>> ranges; };   // ranges: per worker, of the units to walk

// What a route's Worker::chunk answers for one index chunk.  Range: `r` is to be walked (else the chunk holds nothing to walk);
// Last: the window's fetch ends in this chunk, its later chunks are not looked at; Host: the chunk cannot be laid out, the unit is
// the host reader's (EW_RANGE).
enum : unsigned { kChunkRange = 1, kChunkLast = 2, kChunkHost = 4 };

// Every unit's windows as raw ranges, on `nt` threads.  Worker: Worker(Route&, unsigned t), bool ok(),
// unsigned chunk(int32_t tid, int64_t end, uint64_t vbeg, uint64_t vend, RawRange& r).
template <typename Worker, typename Route>
int plan_units(const svt_bam* bam, const svt_summarise_args* args, unsigned nt, Route& route, UnitPlan& plan)
{
    const uint64_t n = args->n_units;
    plan.units.assign(n, UnitRaw());
    plan.ranges.assign(nt, std::vector<RawRange>());
    std::atomic<uint64_t> next(0);
    std::atomic<int> first_rc(SVT_OK);
    run_threads(nt, [&](unsigned t) {
        Worker worker(route, t);
        if (!worker.ok()) { first_rc.store(SVT_ERR_NOMEM); return; }
        std::vector<RawRange>& list = plan.ranges[t];
        for (;;) {
            const uint64_t u0 = next.fetch_add(16);                   // neighbouring units share blocks: they stay on one worker
            if (u0 >= n) return;
            for (uint64_t u = u0; u < std::min(n, u0 + 16); ++u) {
                UnitRaw& U = plan.units[u];
                U.at = list.size();
                U.worker = t;
                const svt_fetch_unit& w = args->windows[u];
                const int32_t tids[2] = {w.tid_a, w.tid_b};
                const int64_t los[2] = {w.lo_a, w.lo_b}, his[2] = {w.hi_a, w.hi_b};
                if (args->breakpoints[u].svtype > SVT_SVTYPE_BND) U.preset = EW_RANGE;       // (the host reader's "bad svtype")
                for (int s = 0; s < 2 && U.preset == EW_OK; ++s) {
                    if (tids[s] < 0 || tids[s] >= (int32_t)bam->ref_names.size()) { U.preset = EW_RANGE; break; }   // ("BAM read error")
                    const int64_t beg = std::max<int64_t>(los[s], 0), end = his[s];
                    if (end <= beg) continue;
                    for (const auto& c : fetch_chunks(*bam, tids[s], beg, end)) {
                        RawRange r{0, 0, 0, 0};
                        const unsigned got = worker.chunk(tids[s], end, c.first, c.second, r);
                        if ((got & kChunkHost) || ((got & kChunkRange) && U.n[s] == 0xFFFF)) { U.preset = EW_RANGE; break; }
                        if (got & kChunkRange) { list.push_back(r); ++U.n[s]; }
                        if (got & kChunkLast) break;
                    }
                }
                if (U.preset != EW_OK) {                               // no walk for this unit
                    list.resize(U.at);
                    U.n[0] = U.n[1] = 0;
                }
            }
        }
    });
    if (first_rc.load() != SVT_OK) return fail(first_rc.load(), "cannot set up the inflate state");
    return SVT_OK;
}

// The blocks the ranges need, side by side: runs of the file's block chain, every block once.  `place(first, last)` lays one run
// out, first block to last, and answers 0 or an error code.
template <typename Place>
int place_runs(const UnitPlan& plan, Place place)
{
    struct Need { uint64_t first, last; };
    std::vector<Need> needs;
    for (const auto& list : plan.ranges)
        for (const RawRange& r : list) needs.push_back(Need{r.first, r.last});
    std::sort(needs.begin(), needs.end(), [](const Need& a, const Need& b) { return a.first < b.first; });
    for (size_t i = 0; i < needs.size();) {
        uint64_t last = needs[i].last;
        size_t j = i + 1;
        while (j < needs.size() && needs[j].first <= last) { last = std::max(last, needs[j].last); ++j; }
        if (const int rc = place(needs[i].first, last)) return rc;
        i = j;
    }
    return SVT_OK;
}

struct Placed { uint64_t at; uint32_t nth; };                         // a block's offset in the arena, and which of the placed blocks it is

// out.ranges and out.units from the raw ranges and the blocks' places.  A block that has no place lies beyond kArenaLimit.
// range_members (the open route's): per range the first and last placed block it lies over.
void finish_ranges(UnitPlan& plan, const std::unordered_map<uint64_t, Placed>& placed, Arena& out,
                   std::vector<std::pair<uint32_t, uint32_t>>* range_members)
{
    const uint64_t n = plan.units.size();
    out.units.resize(n);
    for (uint64_t u = 0; u < n; ++u) {
        UnitRaw& U = plan.units[u];
        const RawRange* list = plan.ranges[U.worker].data() + U.at;
        const uint64_t nr = (uint64_t)U.n[0] + U.n[1];
        const size_t mark = out.ranges.size();
        for (uint64_t k = 0; k < nr; ++k) {
            const RawRange& r = list[k];
            const auto f = placed.find(r.first), l = placed.find(r.last);
            if (f == placed.end() || l == placed.end()) { U.preset = EW_RANGE; break; }
            const uint64_t begin = f->second.at + r.uoff, end = l->second.at + r.end_in_last;
            if (end > kArenaLimit) { U.preset = EW_RANGE; break; }
            // (begin > end: a first record behind the chunk's end -- nothing to walk)
            out.ranges.push_back(Range{(uint32_t)std::min(begin, end), (uint32_t)end});
            if (range_members) range_members->emplace_back(f->second.nth, l->second.nth);
        }
        if (U.preset != EW_OK) {
            out.ranges.resize(mark);
            if (range_members) range_members->resize(mark);
            U.n[0] = U.n[1] = 0;
        }
        out.units[u] = UnitRanges{(uint32_t)mark, {U.n[0], U.n[1]}, U.preset};
    }
    out.ranges.push_back(Range{0, 0});                                // (never an empty array)
}

// ---- the host route: a chunk is inflated and its records are walked up to the one that ends the fetch
struct HostRoute {
    const svt_bam* bam;
    SharedBlocks shared_blocks;
    std::vector<std::vector<std::pair<uint64_t, BlockRef>>> touched;  // per worker: the blocks it loaded
    std::vector<uint64_t> n_records;
    HostRoute(const svt_bam* b, unsigned nt) : bam(b), touched(nt), n_records(nt, 0) {}
};
struct HostWorker {
    Bgzf z;
    std::vector<uint8_t> buf;
    uint64_t& n_records;
    HostWorker(HostRoute& route, unsigned t) : z(route.bam->file, &route.shared_blocks, svt::bam_verify(route.bam)), n_records(route.n_records[t]) { z.touched = &route.touched[t]; }
    bool ok() const { return z.ok(); }
    unsigned chunk(int32_t tid, int64_t end, uint64_t vbeg, uint64_t vend, RawRange& r)
    {
        unsigned got = 0;
        z.seek(vbeg);
        while (z.tell() < vend) {
            const uint64_t at = z.tell();
            const bool beyond_block = z.offset_in_empty_block();       // (the read starts in the block behind it, the range would not)
            uint32_t size = 0;
            const uint8_t* d = next_record(z, buf, size);
            if (!d) {                                                  // end of the data, or a record that is not whole
                if (z.failed() || z.tell() != at) got |= kChunkHost;
                break;
            }
            if ((int32_t)ld32(d) != tid || (int64_t)(int32_t)ld32(d + 4) >= end) { got |= kChunkLast; break; }
            if (!(got & kChunkRange)) {
                r.first = at >> 16;
                r.uoff = (uint32_t)(at & 0xFFFF);
                got |= kChunkRange;
                if (beyond_block) got |= kChunkHost;
            }
            z.last_read(&r.last, &r.end_in_last);
            ++n_records;
        }
        if (z.failed()) got |= kChunkHost;
        return got;
    }
};

// ---- the open route: a chunk is followed through BGZF headers to its end
struct OpenWorker {
    const OpenPlan& f;
    OpenWorker(OpenPlan& plan, unsigned) : f(plan) {}
    bool ok() const { return true; }
    unsigned chunk(int32_t, int64_t, uint64_t vbeg, uint64_t vend, RawRange& r) const
    {
        if (vend <= vbeg) return 0;
        const uint64_t cb = vbeg >> 16, ce = vend >> 16;
        const uint32_t ub = (uint32_t)(vbeg & 0xFFFF), ue = (uint32_t)(vend & 0xFFFF);
        uint64_t coff = cb, src = 0, next = 0;
        uint32_t clen = 0, isize = 0;
        r.first = cb;
        r.uoff = ub;
        // (every step moves forward in the file by a whole member: the walk ends with the file)
        for (;;) {
            if (coff + 18 > f.set.file_size) {                             // the end of the file: the data ends in front of the chunk's end
                if (coff == cb) return 0;                              // (nothing at all: the host reader finds no record either)
                break;
            }
            if (!inf::member_at(f.set.file, f.set.file_size, coff, src, clen, isize, next)) return kChunkHost;
            if (coff == cb && ub > isize) return kChunkHost;           // a first offset beyond the block's bytes
            r.last = coff;
            r.end_in_last = isize;
            if (coff == ce) { r.end_in_last = std::min(ue, isize); break; }   // (an end inside the EOF member: its 0 bytes)
            if (next > ce) return kChunkHost;                          // the chunk's end is not on the block chain
            if (next == ce && ue == 0) break;                          // in-block offset 0 names the block BEHIND the last one needed
            coff = next;
        }
        return kChunkRange;
    }
};

}  // namespace

int build_arena(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out)
{
    if (const int rc = check_arena_args(bam, args, geometry)) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    out = Arena();
    arena_names(bam, args, out);
    const unsigned nt = arena_threads(args, args->n_units);
    const std::unique_ptr<HostRoute> route(new HostRoute(bam, nt));
    UnitPlan plan;
    if (const int rc = plan_units<HostWorker>(bam, args, nt, *route, plan)) return rc;

    // a run's blocks, inflated when a worker walked them, are copied side by side
    std::unordered_map<uint64_t, BlockRef> blocks;
    for (auto& log : route->touched) {
        for (auto& e : log) blocks.emplace(e.first, e.second);
        log.clear();
    }
    std::unordered_map<uint64_t, Placed> placed;
    struct Copy { const BlockData* b; uint64_t at; };
    std::vector<Copy> copies;
    uint64_t total = 0;
    place_runs(plan, [&](uint64_t first, uint64_t last) {
        for (uint64_t coff = first;;) {
            const BlockRef& b = blocks[coff];
            placed[coff] = Placed{total, (uint32_t)copies.size()};
            copies.push_back(Copy{b.get(), total});
            total += b->data.size();
            if (coff == last) return SVT_OK;
            coff = b->next;
        }
    });
    out.bytes.resize(std::min<uint64_t>(total, kArenaLimit) + 8);
    {
        std::atomic<size_t> at(0);
        run_threads(std::min<unsigned>(nt, 16u), [&](unsigned) {
            for (;;) {
                const size_t k = at.fetch_add(8);
                if (k >= copies.size()) return;
                for (size_t c = k; c < std::min(copies.size(), k + 8); ++c)
                    if (copies[c].at + copies[c].b->data.size() <= kArenaLimit && !copies[c].b->data.empty())
                        std::memcpy(out.bytes.data() + copies[c].at, copies[c].b->data.data(), copies[c].b->data.size());
            }
        });
    }
    finish_ranges(plan, placed, out, nullptr);
    for (uint64_t c : route->n_records) out.records_in_ranges += c;
    out.blocks = copies.size();
    out.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    return SVT_OK;
}

int build_arena_open(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, Arena& out, OpenPlan& plan)
{
    if (const int rc = check_arena_args(bam, args, geometry)) return rc;
    const auto t_begin = std::chrono::steady_clock::now();
    out = Arena();
    out.open_ranges = true;
    plan = OpenPlan();
    plan.set.file = bam->file.data;
    plan.set.file_size = bam->file.size;
    arena_names(bam, args, out);
    UnitPlan units;
    if (const int rc = plan_units<OpenWorker>(bam, args, arena_threads(args, args->n_units), plan, units)) return rc;

    // a run's blocks become members to inflate, out of one span of the file; what lies beyond the limit is not placed
    std::unordered_map<uint64_t, Placed> placed;
    uint64_t total = 0;
    const int rc = place_runs(units, [&](uint64_t first, uint64_t last) {
        bgzf::MemberSet::Span span{first, 0, plan.set.compressed_bytes};
        for (uint64_t coff = first;;) {
            uint64_t src = 0, next = 0;
            uint32_t clen = 0, isize = 0;
            if (!inf::member_at(plan.set.file, plan.set.file_size, coff, src, clen, isize, next)) return fail(SVT_ERR_INTERNAL, "build_arena_open: block chain changed under the walk");
            if (total + isize <= kArenaLimit) {
                placed[coff] = Placed{total, (uint32_t)plan.set.members.size()};
                plan.set.members.push_back(inf::Member{span.at + (src - span.file_off), clen, isize, total});
                span.bytes = next - span.file_off;
            }
            total += isize;
            if (coff == last) break;
            coff = next;
        }
        if (span.bytes) { plan.set.spans.push_back(span); plan.set.compressed_bytes += span.bytes; }
        return (int)SVT_OK;
    });
    if (rc) return rc;
    plan.set.arena_bytes = plan.set.members.empty() ? 0 : plan.set.members.back().dst + plan.set.members.back().isize;
    out.bytes.resize(plan.set.arena_bytes + 8);
    out.blocks = plan.set.members.size();
    finish_ranges(units, placed, out, &plan.range_members);
    plan.index_s = out.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    return SVT_OK;
}

uint64_t apply_member_status(const OpenPlan& plan, const std::vector<uint32_t>& status, Arena& out)
{
    std::vector<uint32_t> failed(status.size() + 1, 0);
    for (size_t k = 0; k < status.size(); ++k) failed[k + 1] = failed[k] + (status[k] != inf::INF_OK ? 1u : 0u);
    if (failed.back() == 0) return 0;
    for (auto& U : out.units) {
        if (U.preset != EW_OK) continue;
        const uint32_t nr = (uint32_t)U.n[0] + U.n[1];
        for (uint32_t k = 0; k < nr; ++k) {
            const auto& rm = plan.range_members[U.first + k];
            if (failed[rm.second + 1] != failed[rm.first]) { U.preset = EW_RANGE; U.n[0] = U.n[1] = 0; break; }
        }
    }
    return failed.back();
}

int host_units(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const std::vector<uint64_t>& ids,
               std::vector<svt_record>& records, std::vector<uint64_t>& counts, std::vector<uint8_t>& skipped)
{
    const size_t m = ids.size();
    records.clear();
    counts.assign(m, 0);
    skipped.assign(m, 0);
    if (m == 0) return SVT_OK;
    std::unordered_map<std::string, int32_t> rg_lib;
    for (uint32_t i = 0; i < args->n_read_groups; ++i) rg_lib[args->read_groups[i]] = args->read_group_lib[i];
    std::vector<std::vector<svt_record>> per(m);
    const unsigned nt = arena_threads(args, m);
    const std::unique_ptr<SharedBlocks> shared_blocks(new SharedBlocks());
    std::atomic<size_t> next(0);
    std::mutex err_lock;
    size_t err_at = m;                                                // the first unit (in the units' order) that failed
    int err_rc = SVT_OK;
    std::string err_text;
    run_threads(nt, [&](unsigned) {
        Bgzf z(bam->file, shared_blocks.get(), svt::bam_verify(bam));
        std::vector<uint8_t> buf;
        UnitOut unit;
        Workspace ws;
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= m) return;
            std::string err;
            const int rc = z.ok() ? evidence_unit(*bam, z, buf, *args, *geometry, rg_lib, ids[k], ws, unit, err) : SVT_ERR_NOMEM;
            if (rc != SVT_OK) {
                std::lock_guard<std::mutex> g(err_lock);
                if (k < err_at) { err_at = k; err_rc = rc; err_text = z.ok() ? err : "cannot set up the inflate state"; }
                continue;
            }
            per[k] = unit.recs;
            skipped[k] = unit.skipped ? 1 : 0;
        }
    });
    if (err_rc != SVT_OK) return fail(err_rc, err_text);
    for (size_t k = 0; k < m; ++k) {
        counts[k] = per[k].size();
        records.insert(records.end(), per[k].begin(), per[k].end());
    }
    return SVT_OK;
}

}  // namespace ew
}  // namespace svt

// svt_trim()'s share of this file: the pooled huge-page buffers of the gather (up to SVT_READER_POOL_MB, 1 GiB by default)
extern "C" void svt_reads_trim() { BufferPool::get().trim(); }      // (internal: not in include/svtyper_reads.h)

extern "C" {

static int svt_bam_open_impl(const char* path, svt_bam** out)
{
    if (!path || !out) return fail(SVT_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<svt_bam> b(new svt_bam());
    b->path = path;
    if (!b->file.open(b->path)) return fail(SVT_ERR_INVALID, std::string("cannot open ") + path);
    Bgzf z(b->file);
    if (!z.ok()) return fail(SVT_ERR_NOMEM, "cannot set up the inflate state");
    uint8_t magic[4];
    z.seek(0);
    auto rd32 = [&](int32_t& v) {
        uint8_t t[4];
        if (z.read(t, 4) != 4) return false;
        v = (int32_t)((uint32_t)t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24));
        return true;
    };
    int32_t l_text = 0, n_ref = 0;
    if (z.read(magic, 4) != 4 || std::memcmp(magic, "BAM\1", 4) != 0 || !rd32(l_text) || l_text < 0)
        return fail(SVT_ERR_INVALID, std::string(path) + " is not a BAM file");
    b->text.resize((size_t)l_text);
    if (l_text && z.read(&b->text[0], (size_t)l_text) != (size_t)l_text) return fail(SVT_ERR_INVALID, "truncated BAM header");
    b->text = b->text.c_str();   // cut at the first NUL
    if (!rd32(n_ref) || n_ref < 0) return fail(SVT_ERR_INVALID, "truncated BAM header");
    for (int32_t i = 0; i < n_ref; ++i) {
        int32_t l_name = 0, l_ref = 0;
        if (!rd32(l_name) || l_name <= 0) return fail(SVT_ERR_INVALID, "truncated BAM header");
        std::string name((size_t)l_name, '\0');
        if (z.read(&name[0], (size_t)l_name) != (size_t)l_name || !rd32(l_ref)) return fail(SVT_ERR_INVALID, "truncated BAM header");
        name.resize((size_t)l_name - 1);
        b->tid_of[name] = i;
        b->ref_names.push_back(name);
        b->ref_lengths.push_back(l_ref);
    }
    b->first_record = z.tell();
    // index: <path>.bai, the .bai next to the file, <path>.csi, the .csi next to it.  .bai first: a call that found its index
    // before this list grew reads the same file as before (htslib would take a .csi first; the answers are the same).  What a
    // file is, its magic says, not its name.
    std::string stem = b->path;
    const size_t dot = stem.rfind('.');
    if (dot != std::string::npos) stem = stem.substr(0, dot);
    const std::string cand[4] = {b->path + ".bai", stem + ".bai", b->path + ".csi", stem + ".csi"};
    for (const std::string& p : cand) {
        FILE* f = std::fopen(p.c_str(), "rb");
        if (!f) continue;
        std::vector<uint8_t> data;
        uint8_t tmp[65536];
        size_t n;
        while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        std::fclose(f);
        std::string err;
        if (!svt::bamidx::load(data.data(), data.size(), p, b->index, err)) return fail(SVT_ERR_INVALID, err);
        break;
    }
    if (!b->has_index()) return fail(SVT_ERR_INVALID, std::string("no .bai index found for ") + path + " (nor a .csi)");
    if (b->index.refs.size() < b->ref_names.size()) b->index.refs.resize(b->ref_names.size());
    *out = b.release();
    return SVT_OK;
}

int svt_bam_open(const char* path, svt_bam** out)
{
    return guarded([&] { return svt_bam_open_impl(path, out); });
}

void svt_bam_close(svt_bam* bam) { delete bam; }

int svt_bam_index_info(const svt_bam* bam, int* kind, int* min_shift, int* depth)
{
    if (!bam) return fail(SVT_ERR_INVALID, "null argument");
    if (kind) *kind = bam->index.kind;
    if (min_shift) *min_shift = bam->index.min_shift;
    if (depth) *depth = bam->index.depth;
    return SVT_OK;
}

int32_t svt_bam_n_references(const svt_bam* bam) { return bam ? (int32_t)bam->ref_names.size() : 0; }

const char* svt_bam_reference_name(const svt_bam* bam, int32_t tid)
{
    return (bam && tid >= 0 && tid < (int32_t)bam->ref_names.size()) ? bam->ref_names[tid].c_str() : nullptr;
}

int64_t svt_bam_reference_length(const svt_bam* bam, int32_t tid)
{
    return (bam && tid >= 0 && tid < (int32_t)bam->ref_lengths.size()) ? bam->ref_lengths[tid] : -1;
}

int32_t svt_bam_tid(const svt_bam* bam, const char* name)
{
    if (!bam || !name) return -1;
    auto it = bam->tid_of.find(name);
    return it == bam->tid_of.end() ? -1 : it->second;
}

const char* svt_bam_header_text(const svt_bam* bam) { return bam ? bam->text.c_str() : nullptr; }

// What the workers' results are gathered into: the three arrays of svt_summaries (elements: 128-byte summaries) or of
// svt_evidence (elements: 16-byte records made from the summaries by svt_geometry_math.h, `geometry` != nullptr).
struct GatherOut {
    uint64_t** offset;
    void** elements;
    uint8_t** skipped;
    size_t element_bytes;
};

static void free_gathered(uint64_t*& offset, void*& elements, uint8_t*& skipped)
{
    std::free(offset);
    if (elements && !BufferPool::get().release_tracked(elements)) std::free(elements);
    std::free(skipped);
    offset = nullptr;
    elements = nullptr;
    skipped = nullptr;
}

static int summarise_units(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, GatherOut out)
{
    if (!bam || !args) return fail(SVT_ERR_INVALID, "null argument");
    *out.offset = nullptr;
    *out.elements = nullptr;
    *out.skipped = nullptr;
    if (geometry && (geometry->n_libs == 0 || geometry->n_libs > 65536 || !geometry->lib_flank))
        return fail(SVT_ERR_INVALID, "n_libs must be 1..65536 with a flank per library");
    const uint64_t n = args->n_units;
    if (n && (!args->windows || !args->breakpoints)) return fail(SVT_ERR_INVALID, "null unit arrays");
    std::unordered_map<std::string, int32_t> rg_lib;
    for (uint32_t i = 0; i < args->n_read_groups; ++i) rg_lib[args->read_groups[i]] = args->read_group_lib[i];

    const bool trace = std::getenv("SVT_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace)
            std::fprintf(stderr, "[svt_bam_summarise] %-10s %8.1f ms\n", what,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
    };
    std::vector<UnitSpan> outs(n);
    // by default one usable CPU is left to the caller's other thread (the drivers parse the next chunk of the VCF while this
    // runs: pipeline.ChunkPipeline).  A call whose CPU time fits well inside one period of a cgroup quota is a burst
    // (svt_host_cpus.h) and runs on up to 48 physical cores instead: its CPU time is what the last calls on this file
    // measured per unit (+ 30 %), or 350 us per unit when there is none yet -- a window pair at 30x costs 210 us on the
    // 9575F, mostly inflate.  (290 whole-genome-like sites: 97 ms of CPU time, 7.9 -> 2.4 ms; the fixture's 21 100 units:
    // 0.45 s, 31 -> ms -- 16 CPUs for a tenth of a second are the same allowance as 48 for a thirtieth.)
    // (a handle that has not measured anything yet -- every run of a driver opens its own -- goes by what the last call on
    // ANY file of this process measured)
    double known = bam->cpu_s_per_unit.load(std::memory_order_relaxed);
    if (!(known > 0.0)) known = g_cpu_s_per_unit.load(std::memory_order_relaxed);
    const double est_cpu_s = (double)n * (known > 0.0 ? 1.3 * known : 350e-6);
    unsigned nt = args->n_threads > 0 ? (unsigned)args->n_threads : std::max(1u, svt::burst_threads(est_cpu_s, 48u) - 1u);
    nt = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nt ? nt : 1, n ? n : 1));
    // Consecutive units stay on one worker: neighbouring sites share BGZF blocks, and the worker's own slots serve them
    // without a lock (what a worker re-reads at the start of a run comes from SharedBlocks).  A grab is a long run while
    // there is plenty left and shrinks towards the end, where balance matters: half of an even share of what remains,
    // between 4 (fewer when the call is too small to feed every worker that way) and 64 units (guided self-scheduling).
    const uint64_t min_grab = std::max<uint64_t>(1, std::min<uint64_t>(4, n / (4ull * nt)));
    std::atomic<uint64_t> next(0);
    auto claim = [&](uint64_t& lo, uint64_t& hi) {
        uint64_t at = next.load(std::memory_order_relaxed);
        for (;;) {
            if (at >= n) return false;
            const uint64_t take = std::min<uint64_t>(n - at, std::max<uint64_t>(min_grab, std::min<uint64_t>(64, (n - at) / (2ull * nt))));
            if (next.compare_exchange_weak(at, at + take, std::memory_order_relaxed)) {
                lo = at;
                hi = at + take;
                return true;
            }
        }
    };
    std::atomic<int> first_rc(SVT_OK);
    std::mutex err_lock;
    std::string first_err;
    std::vector<std::unique_ptr<SummaryArena>> arenas(nt);
    const std::unique_ptr<SharedBlocks> shared_blocks(new SharedBlocks());
    struct WorkerStat { double start_s = 0, busy_s = 0, cpu_s = 0, inflate_s = 0; uint64_t units = 0, grabs = 0, inflated = 0, shared = 0, ahead = 0; };
    std::vector<WorkerStat> stats(nt);
    auto worker = [&](unsigned t) {
        const auto w_begin = std::chrono::steady_clock::now();
        stats[t].start_s = std::chrono::duration<double>(w_begin - t_begin).count();
        Bgzf z(bam->file, shared_blocks.get(), svt::bam_verify(bam));
        struct Report {
            WorkerStat& st; Bgzf& z; std::chrono::steady_clock::time_point t0; double cpu0;
            ~Report() { st.cpu_s = thread_cpu_seconds() - cpu0; st.busy_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); st.inflate_s = z.inflate_s; st.inflated = z.n_inflated; st.shared = z.n_shared_hits; st.ahead = z.n_ahead; }
        } report{stats[t], z, w_begin, thread_cpu_seconds()};
        std::vector<uint8_t> buf;
        UnitOut unit;
        Workspace ws;
        arenas[t].reset(new SummaryArena());
        if (!z.ok()) {
            std::lock_guard<std::mutex> g(err_lock);
            if (first_rc.exchange(SVT_ERR_NOMEM) == SVT_OK) first_err = "cannot set up the inflate state";
            return;
        }
        for (;;) {   // consecutive units stay on one thread: neighbouring sites share BGZF blocks (and its cache)
            uint64_t u0, u1;
            if (!claim(u0, u1)) return;
            stats[t].grabs += 1;
            stats[t].units += u1 - u0;
            for (uint64_t u = u0; u < u1; ++u) {
                if (first_rc.load(std::memory_order_relaxed) != SVT_OK) return;
                std::string err;
                int rc;
                if (geometry) {      // the predicates of the device stage, here: 16 bytes per fragment leave the reader
                    rc = evidence_unit(*bam, z, buf, *args, *geometry, rg_lib, u, ws, unit, err);
                } else {
                    rc = process_unit(*bam, z, buf, *args, rg_lib, u, ws, unit, err, [&](const svt_fragment& f) { unit.frags.push_back(f); return true; });
                }
                if (rc == SVT_OK) {
                    outs[u].count = geometry ? unit.recs.size() : unit.frags.size();
                    outs[u].skipped = unit.skipped;
                    outs[u].data = geometry ? arenas[t]->append(unit.recs.data(), unit.recs.size() * sizeof(svt_record))
                                            : arenas[t]->append(unit.frags.data(), unit.frags.size() * sizeof(svt_fragment));
                    if (outs[u].count && !outs[u].data) { rc = SVT_ERR_NOMEM; err = "out of host memory"; }
                }
                if (rc != SVT_OK) {
                    std::lock_guard<std::mutex> g(err_lock);
                    if (first_rc.exchange(rc) == SVT_OK) first_err = err;
                    return;
                }
            }
        }
    };
    run_threads(nt, worker);
    if (first_rc.load() != SVT_OK) return fail(first_rc.load(), first_err);
    lap("units");
    {   // what a unit of this file costs: half the last call, half the calls before it
        double cpu = 0.0;
        for (const auto& w : stats) cpu += w.cpu_s;
        if (n && cpu > 0.0) {
            const double now = cpu / (double)n, before = bam->cpu_s_per_unit.load(std::memory_order_relaxed);
            bam->cpu_s_per_unit.store(before > 0.0 ? 0.5 * (before + now) : now, std::memory_order_relaxed);
            g_cpu_s_per_unit.store(now, std::memory_order_relaxed);
        }
        svt::note_cpu_s(cpu);
    }
    if (trace) {
        WorkerStat sum, longest;
        double first_start = 1e9, last_start = 0, first_end = 1e9, last_end = 0;
        for (const auto& w : stats) {
            first_start = std::min(first_start, w.start_s); last_start = std::max(last_start, w.start_s);
            first_end = std::min(first_end, w.start_s + w.busy_s); last_end = std::max(last_end, w.start_s + w.busy_s);
            sum.busy_s += w.busy_s; sum.cpu_s += w.cpu_s; sum.inflate_s += w.inflate_s; sum.inflated += w.inflated; sum.shared += w.shared; sum.grabs += w.grabs; sum.ahead += w.ahead;
            if (w.busy_s > longest.busy_s) longest = w;
        }
        std::fprintf(stderr, "[svt_bam_summarise] workers started %.2f .. %.2f ms, finished %.2f .. %.2f ms\n", first_start * 1e3, last_start * 1e3, first_end * 1e3, last_end * 1e3);
        std::fprintf(stderr, "[svt_bam_summarise] %u workers: CPU %.1f ms, busy %.1f ms in all (longest %.1f ms: %llu units in %llu grabs, %.1f ms inflating), %llu grabs, "
                             "%llu blocks inflated in %.1f ms (%llu of them ahead for others), %llu taken from other workers\n", nt, sum.cpu_s * 1e3, sum.busy_s * 1e3, longest.busy_s * 1e3,
                     (unsigned long long)longest.units, (unsigned long long)longest.grabs, longest.inflate_s * 1e3, (unsigned long long)sum.grabs,
                     (unsigned long long)sum.inflated, sum.inflate_s * 1e3, (unsigned long long)sum.ahead, (unsigned long long)sum.shared);
    }

    uint64_t total = 0;
    for (const auto& o : outs) total += o.count;
    uint64_t* offsets = static_cast<uint64_t*>(std::malloc((n + 1) * sizeof(uint64_t)));
    void* elements = nullptr;
    {   // from the pool of huge-page mappings when it is large (1.4 GB for 10 M summaries), malloc otherwise
        const size_t bytes = std::max<uint64_t>(total, 1) * out.element_bytes;
        elements = bytes >= (4u << 20) ? BufferPool::get().acquire_tracked(bytes) : std::malloc(bytes);
    }
    uint8_t* skipped = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(n, 1)));
    if (!offsets || !elements || !skipped) {
        free_gathered(offsets, elements, skipped);
        return fail(SVT_ERR_NOMEM, "out of host memory");
    }
    uint64_t off = 0;
    for (uint64_t u = 0; u < n; ++u) {
        offsets[u] = off;
        off += outs[u].count;
        skipped[u] = outs[u].skipped ? 1 : 0;
    }
    offsets[n] = off;
    {   // gather the per-unit vectors into the flat array on the same threads
        std::atomic<uint64_t> nextu(0);
        auto copier = [&]() {
            for (;;) {
                const uint64_t u0 = nextu.fetch_add(256);
                if (u0 >= n) return;
                for (uint64_t u = u0; u < std::min(n, u0 + 256); ++u)
                    if (outs[u].count)
                        std::memcpy(static_cast<uint8_t*>(elements) + offsets[u] * out.element_bytes, outs[u].data, outs[u].count * out.element_bytes);
            }
        };
        run_threads(std::min(nt, 32u), [&](unsigned) { copier(); });
    }
    *out.offset = offsets;
    *out.elements = elements;
    *out.skipped = skipped;
    lap("gather");
    arenas.clear();
    lap("release");
    return SVT_OK;
}

int svt_bam_summarise(const svt_bam* bam, const svt_summarise_args* args, svt_summaries* out)
{
    return guarded([&] {
        if (!out) return fail(SVT_ERR_INVALID, "null argument");
        svt::VerifyScope verify_scope(bam);
        void* elements = nullptr;
        const int rc = summarise_units(bam, args, nullptr, GatherOut{&out->frag_offset, &elements, &out->skipped, sizeof(svt_fragment)});
        out->fragments = static_cast<svt_fragment*>(elements);
        return rc;
    });
}

void svt_summaries_free(svt_summaries* s)
{
    if (!s) return;
    void* elements = s->fragments;
    free_gathered(s->frag_offset, elements, s->skipped);
    s->fragments = nullptr;
}

int svt_bam_evidence(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out)
{
    return guarded([&] {
        if (!out || !geometry) return fail(SVT_ERR_INVALID, "null argument");
        svt::VerifyScope verify_scope(bam);
        void* elements = nullptr;
        const int rc = summarise_units(bam, args, geometry, GatherOut{&out->rec_offset, &elements, &out->skipped, sizeof(svt_record)});
        out->records = static_cast<svt_record*>(elements);
        return rc;
    });
}

void svt_evidence_free(svt_evidence* e)
{
    if (!e) return;
    void* elements = e->records;
    free_gathered(e->rec_offset, elements, e->skipped);
    e->records = nullptr;
}

// `dump` (svt_bam_evidence_dump_walk_host): the walk also leaves its source rows, and the dump rules run over them and `verdicts`
static int dump_units_host(const svt::ew::Arena& arena, const std::vector<std::vector<svt::ew::SrcRow>>& src, const std::vector<uint32_t>& status,
                           const uint64_t* rec_offset, const uint8_t* verdicts, svt_evidence_dump* dump);

static int svt_bam_evidence_walk_host_impl(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                           svt_evidence* out, uint8_t* out_of_envelope, uint32_t* kept_reads, bool open_ranges,
                                           const uint8_t* verdicts = nullptr, uint64_t n_verdicts = 0, svt_evidence_dump* dump = nullptr)
{
    if (!out || !out_of_envelope) return fail(SVT_ERR_INVALID, "null argument");
    svt::VerifyScope verify_scope(bam);
    out->rec_offset = nullptr;
    out->records = nullptr;
    out->skipped = nullptr;
    if (dump) *dump = svt_evidence_dump{};
    svt::ew::Arena arena;
    if (open_ranges) {
        svt::ew::OpenPlan plan;
        if (const int rc = svt::ew::build_arena_open(bam, args, geometry, arena, plan)) return rc;
        std::vector<uint32_t> member_status;
        const size_t m = plan.set.members.size();
        svt::bgzf::inflate_members_host(plan.set, arena.bytes.data(), std::min<unsigned>(svt::ew::arena_threads(args, m), (unsigned)std::max<size_t>(m, 1)),
                                        svt::bgzf::Decoder::one_source, svt::bgzf::Crc::library, svt::bam_verify(bam), member_status);
        svt::ew::apply_member_status(plan, member_status, arena);
    } else if (const int rc = svt::ew::build_arena(bam, args, geometry, arena)) return rc;
    const uint64_t n = args->n_units;
    const svt::ew::Params P = arena.params(args, geometry);
    std::vector<std::vector<svt::Record4>> per(n);
    std::vector<std::vector<svt::ew::SrcRow>> src(dump ? n : 0);
    std::vector<uint32_t> status(n, 0);
    std::atomic<uint64_t> next(0);
    const unsigned nt = svt::ew::arena_threads(args, n);
    run_threads(nt, [&](unsigned) {
        std::unique_ptr<svt::ew::UnitScratch> S(new svt::ew::UnitScratch());
        std::vector<svt::Record4> rows(svt::ew::kMaxReads);    // (a unit has at most one row per kept read)
        std::vector<svt::ew::SrcRow> src_rows(dump ? svt::ew::kMaxReads : 0);
        // the deep tier's scratch and tables, from the heap once this thread meets a unit that needs them
        std::unique_ptr<svt::ew::DeepScratch> D;
        std::unique_ptr<uint64_t[]> slice;
        for (;;) {
            const uint64_t u = next.fetch_add(1);
            if (u >= n) return;
            if (dump) svt::ew::walk_unit<svt::ew::HostCtx, svt::ew::UnitScratch, true>(P, u, *S, S->tables(), rows.data(), src_rows.data());
            else svt::ew::walk_unit<svt::ew::HostCtx>(P, u, *S, S->tables(), rows.data());
            uint32_t st = S->status, n_reads = S->n_reads, n_rows = S->n_rows;
            if (svt::ew::deep_tier_unit(st, n_reads)) {
                if (!D) {
                    D.reset(new svt::ew::DeepScratch());
                    slice.reset(new uint64_t[svt::ew::kDeepSliceBytes / sizeof(uint64_t)]);
                    rows.resize(svt::ew::kMaxReadsDeep);
                    if (dump) src_rows.resize(svt::ew::kMaxReadsDeep);
                }
                const svt::ew::Tables<uint32_t> T = svt::ew::deep_tables(reinterpret_cast<uint8_t*>(slice.get()));
                if (dump) svt::ew::walk_unit<svt::ew::HostCtx, svt::ew::DeepScratch, true>(P, u, *D, T, rows.data(), src_rows.data());
                else svt::ew::walk_unit<svt::ew::HostCtx>(P, u, *D, T, rows.data());
                st = D->status; n_reads = D->n_reads; n_rows = D->n_rows;
            }
            status[u] = st;
            if (kept_reads) kept_reads[u] = n_reads;
            if (st == svt::ew::EW_OK) per[u].assign(rows.begin(), rows.begin() + n_rows);
            if (dump && st == svt::ew::EW_OK) src[u].assign(src_rows.begin(), src_rows.begin() + n_rows);
        }
    });
    uint64_t total = 0;
    for (const auto& v : per) total += v.size();
    out->rec_offset = static_cast<uint64_t*>(std::malloc((n + 1) * sizeof(uint64_t)));
    out->records = static_cast<svt_record*>(std::malloc(std::max<uint64_t>(total, 1) * sizeof(svt_record)));
    out->skipped = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(n, 1)));
    if (!out->rec_offset || !out->records || !out->skipped) {
        svt_evidence_free(out);
        return fail(SVT_ERR_NOMEM, "out of host memory");
    }
    uint64_t off = 0;
    for (uint64_t u = 0; u < n; ++u) {
        out->rec_offset[u] = off;
        if (!per[u].empty()) std::memcpy(out->records + off, per[u].data(), per[u].size() * sizeof(svt_record));
        off += per[u].size();
        out->skipped[u] = status[u] == svt::ew::EW_SKIPPED ? 1 : 0;
        out_of_envelope[u] = status[u] >= svt::ew::EW_RANGE ? (uint8_t)status[u] : 0;
    }
    out->rec_offset[n] = off;
    if (dump) {
        if (n_verdicts != off || (off && !verdicts)) {
            svt_evidence_free(out);
            return fail(SVT_ERR_INVALID, "svt_bam_evidence_dump_walk_host: one verdict byte per record of svt_bam_evidence_walk_host on the same arguments");
        }
        if (const int rc = dump_units_host(arena, src, status, out->rec_offset, verdicts, dump)) {
            svt_evidence_free(out);
            return rc;
        }
    }
    return SVT_OK;
}

// the dump rules on one lane, unit after unit
static int dump_units_host(const svt::ew::Arena& arena, const std::vector<std::vector<svt::ew::SrcRow>>& src, const std::vector<uint32_t>& status,
                           const uint64_t* rec_offset, const uint8_t* verdicts, svt_evidence_dump* dump)
{
    namespace dr = svt::dr;
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = src.size();
    dump->unit_offset = static_cast<uint64_t*>(std::calloc(n + 1, sizeof(uint64_t)));
    dump->unit_host = static_cast<uint8_t*>(std::calloc(std::max<uint64_t>(n, 1), 1));
    if (!dump->unit_offset || !dump->unit_host) { svt_evidence_dump_free(dump); return fail(SVT_ERR_NOMEM, "out of host memory"); }
    std::vector<std::vector<uint32_t>> slot_len(n);
    std::vector<std::vector<uint8_t>> slot_state(n);
    auto unit_of = [&](uint64_t u) {
        dr::Unit U;
        U.arena = arena.bytes.data();
        U.arena_len = arena.bytes.size();
        U.rows = src[u].data();
        U.verdicts = verdicts + rec_offset[u];
        U.n_rows = (uint32_t)src[u].size();
        U.slot_len = slot_len[u].data();
        U.slot_state = slot_state[u].data();
        return U;
    };
    for (uint64_t u = 0; u < n; ++u) {
        dump->unit_offset[u + 1] = dump->unit_offset[u];
        if (status[u] >= svt::ew::EW_RANGE) { dump->unit_host[u] = 1; ++dump->units_host; continue; }   // outside the walk's envelope
        if (src[u].empty()) continue;                                                                    // skipped, or without reads
        slot_len[u].assign(2 * src[u].size(), 0);
        slot_state[u].assign(2 * src[u].size(), 0);
        uint64_t bytes = 0;
        uint32_t reads = 0;
        if (!dr::size_unit<svt::ew::HostCtx>(unit_of(u), bytes, reads)) {                                       // outside the dump's
            dump->unit_host[u] = 1;
            ++dump->units_host;
            ++dump->units_outside_dump;
            slot_len[u].clear();
            continue;
        }
        dump->unit_offset[u + 1] += bytes;
        dump->n_reads += reads;
        ++dump->units_dumped;
    }
    dump->n_bytes = dump->unit_offset[n];
    dump->bytes = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(dump->n_bytes, 1)));
    if (!dump->bytes) { svt_evidence_dump_free(dump); return fail(SVT_ERR_NOMEM, "out of host memory"); }
    std::vector<uint32_t> slot_off;
    for (uint64_t u = 0; u < n; ++u) {
        if (slot_len[u].empty() || dump->unit_offset[u + 1] == dump->unit_offset[u]) continue;
        const dr::Unit U = unit_of(u);
        uint32_t partial[1];
        slot_off.assign(slot_len[u].size(), 0);
        dr::place_slots<svt::ew::HostCtx>(U.slot_len, slot_off.data(), 2 * U.n_rows, partial);
        for (uint32_t k = 0; k < 2 * U.n_rows; ++k) {
            if (!U.slot_len[k]) continue;
            if (!dr::emit_read<svt::ew::HostCtx>(U.arena, U.arena_len, U.rows[k / 2].rec[k & 1], U.slot_state[k], dump->bytes + dump->unit_offset[u] + slot_off[k], U.slot_len[k])) {
                svt_evidence_dump_free(dump);
                return fail(SVT_ERR_INTERNAL, "svt_bam_evidence_dump_walk_host: a read does not give the bytes it was sized for");
            }
        }
    }
    dump->dump_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return SVT_OK;
}

void svt_evidence_dump_free(svt_evidence_dump* d)
{
    if (!d) return;
    std::free(d->bytes);
    std::free(d->unit_offset);
    std::free(d->unit_host);
    d->bytes = nullptr;
    d->unit_offset = nullptr;
    d->unit_host = nullptr;
}

int svt_bam_evidence_dump_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const uint8_t* verdicts,
                                    uint64_t n_verdicts, svt_evidence* out, uint8_t* out_of_envelope, svt_evidence_dump* dump)
{
    return guarded([&] {
        if (!dump) return fail(SVT_ERR_INVALID, "null argument");
        return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, nullptr, false, verdicts, n_verdicts, dump);
    });
}

int svt_bam_evidence_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out,
                               uint8_t* out_of_envelope, uint32_t* kept_reads)
{
    return guarded([&] { return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, kept_reads, false); });
}

int svt_bam_evidence_walk_open_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out,
                                    uint8_t* out_of_envelope, uint32_t* kept_reads)
{
    return guarded([&] { return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, kept_reads, true); });
}

static int svt_bgzf_inflate_host_impl(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                      const uint64_t* out_off, uint32_t* status, bool verify)
{
    svt::bgzf::MemberSet set;
    if (const int rc = svt::bgzf::bgzf_members(data, len, block_off, n, out, out_off, status, set)) return rc;
    // (the one-source decoder and CRC on this thread, as the device entry's kernels run them; nothing is counted)
    svt::VerifyTally uncounted;
    std::vector<uint32_t> st;
    svt::bgzf::inflate_members_host(set, out, 1, svt::bgzf::Decoder::one_source, svt::bgzf::Crc::one_source, verify ? &uncounted : nullptr, st);
    if (n) std::memcpy(status, st.data(), n * sizeof(uint32_t));
    return SVT_OK;
}

int svt_bgzf_inflate_host(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out, const uint64_t* out_off,
                          uint32_t* status)
{
    return guarded([&] { return svt_bgzf_inflate_host_impl(data, len, block_off, n, out, out_off, status, false); });
}

int svt_bgzf_inflate_host_verified(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                   const uint64_t* out_off, uint32_t* status)
{
    return guarded([&] { return svt_bgzf_inflate_host_impl(data, len, block_off, n, out, out_off, status, true); });
}

int svt_bgzf_crc32_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t* crc)
{
    return guarded([&]() -> int {
        if (const int rc = svt::crc_check_offsets(bytes, off, n, crc)) return rc;
        std::unique_ptr<svt::crc::Scratch> C(new svt::crc::Scratch());
        for (uint64_t k = 0; k < n; ++k) crc[k] = svt::crc::crc_member<svt::crc::HostCtx>(bytes + off[k], (uint32_t)(off[k + 1] - off[k]), svt::crc_tables(), *C);
        return SVT_OK;
    });
}

// svt_deflate.h on this thread, member by member: each into a slot of its own first, since its size is known only afterwards
int svt_bgzf_deflate_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off)
{
    namespace dfl = svt::dfl;
    return guarded([&]() -> int {
        uint64_t slots = 0;
        if (const int rc = svt::deflate_check_args(bytes, off, n, out, out_off, slots)) return rc;
        std::unique_ptr<dfl::Scratch<dfl::HostCtx::kWidth>> S(new dfl::Scratch<dfl::HostCtx::kWidth>());
        std::unique_ptr<svt::crc::Scratch> C(new svt::crc::Scratch());
        std::vector<uint8_t> slot(dfl::slot_bytes(dfl::kMaxPayload));
        uint64_t at = 0;
        out_off[0] = 0;
        for (uint64_t k = 0; k < n; ++k) {
            const uint8_t* p = bytes + off[k];
            const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
            const uint32_t clen = dfl::deflate_member<dfl::HostCtx>(p, len, slot.data() + dfl::kHeaderBytes, dfl::cdata_bound(len), *S);
            if (!clen) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: a payload was refused");
            const uint64_t size = (uint64_t)dfl::kHeaderBytes + clen + dfl::kTrailerBytes;
            if (size > capacity - at) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: capacity is below what the members need");
            const uint32_t crc = svt::crc::crc_member<svt::crc::HostCtx>(p, len, svt::crc_tables(), *C);
            for (uint32_t i = 0; i < dfl::kHeaderBytes; ++i) slot[i] = dfl::header_byte(i, clen);
            for (uint32_t i = 0; i < dfl::kTrailerBytes; ++i) slot[dfl::kHeaderBytes + clen + i] = dfl::trailer_byte(i, crc, len);
            std::memcpy(out + at, slot.data(), size);
            at += size;
            out_off[k + 1] = at;
        }
        return SVT_OK;
    });
}

int svt_bam_set_verify(svt_bam* bam, int on)
{
    return guarded([&]() -> int {
        if (!bam) return fail(SVT_ERR_INVALID, "null argument");
        bam->verify.store(on ? 1 : 0);
        return SVT_OK;
    });
}

int svt_bam_get_verify(const svt_bam* bam) { return bam ? bam->verify.load() : 0; }

int svt_bgzf_verify_stats(svt_bgzf_verify_counts* out)
{
    return guarded([&]() -> int {
        if (!out) return fail(SVT_ERR_INVALID, "null argument");
        *out = g_verify_stats;
        return SVT_OK;
    });
}

uint32_t svt_evidence_walk_capacity(int which)
{
    switch (which) {
    case SVT_WALK_CAP_READS: return svt::ew::kMaxReadsDeep;
    case SVT_WALK_CAP_READS_LDS: return svt::ew::kMaxReads;
    case SVT_WALK_CAP_NAME: return svt::ew::kMaxName;
    case SVT_WALK_CAP_CIGAR: return svt::ew::kMaxCigar;
    case SVT_WALK_CAP_SA_ENTRIES: return svt::ew::kMaxSaEntries;
    case SVT_WALK_CAP_SA_BYTES: return svt::ew::kMaxSaBytes;
    case SVT_WALK_CAP_RECORD: return svt::ew::kMaxRecord;
    default: return 0;
    }
}

static int svt_bam_scan_library_impl(const svt_bam* bam, uint32_t n_read_groups, const char* const* read_groups, int64_t num_samp,
                         svt_library_scan* out)
{
    if (!bam || !out || (n_read_groups && !read_groups)) return fail(SVT_ERR_INVALID, "null argument");
    *out = svt_library_scan{};
    std::set<std::string> rgset;
    for (uint32_t i = 0; i < n_read_groups; ++i) rgset.insert(read_groups[i]);
    Bgzf z(bam->file, nullptr, svt::bam_verify(bam));
    if (!z.ok()) return fail(SVT_ERR_NOMEM, "cannot set up the inflate state");
    std::vector<uint8_t> buf;
    Record r;
    // 1 in the set, 0 not in the set, -1 no usable RG tag (an error where the reference calls get_tag)
    auto in_library = [&](const Record& rec) -> int {
        rr::Tags tags;
        uint32_t behind_rg = 0;
        const char* rg = read_group(rec, tags, behind_rg);
        if (!rg) return -1;
        return rgset.count(rg) ? 1 : 0;
    };
    auto no_rg = [&](const Record& rec) { return fail(SVT_ERR_INVALID, "read without a usable RG tag: " + rec.name_str()); };
    auto query_length = [](const Record& rec) {
        int64_t n = 0;
        for (uint32_t k = 0; k < rec.n_cigar; ++k) {
            const uint32_t c = ld32(rec.cigar() + 4 * k);
            if (rr::op_query(c & 0xF) || (c & 0xF) == 4) n += (int64_t)(c >> 4);
        }
        return n;
    };

    // calc_read_length (parsers.py:516-528)
    z.seek(bam->first_record);
    // (an indexed file is walked reference by reference, pysam's IteratorRowAllRefs: the unplaced unmapped reads a
    //  coordinate-sorted BAM ends with -- reference id -1 -- are never seen by the reference)
    for (int64_t seen = 0; read_record(z, buf, r) && r.tid >= 0;) {
        const int in = in_library(r);
        if (in < 0) return no_rg(r);
        if (!in) continue;
        out->read_length = std::max(out->read_length, query_length(r));
        if (seen == 10000) break;
        ++seen;
    }
    // calc_insert_hist (parsers.py:534-576)
    // keys in order of first occurrence, like the reference's Counter: its mean / sd are sums in that order
    std::vector<int64_t> hist_keys;
    std::vector<uint64_t> hist_counts;
    std::unordered_map<int64_t, size_t> hist_slot;
    z.seek(bam->first_record);
    for (int64_t n = 0; read_record(z, buf, r) && r.tid >= 0;) {
        if ((r.flag & 0x10) || !(r.flag & 0x20) || (r.flag & (0x4 | 0x8)) || (r.flag & (0x100 | 0x800))) continue;
        if (r.tlen() <= 0) continue;
        const int in = in_library(r);
        if (in < 0) return no_rg(r);
        if (!in) continue;
        auto slot = hist_slot.find(r.tlen());
        if (slot == hist_slot.end()) {
            hist_slot.emplace(r.tlen(), hist_keys.size());
            hist_keys.push_back(r.tlen());
            hist_counts.push_back(1);
        } else {
            ++hist_counts[slot->second];
        }
        if (++n == num_samp) break;    // parsers.py:571-573: tested after the increment, so -n 0 scans the whole file
    }
    // calc_lib_prevalence (parsers.py:501-513)
    z.seek(bam->first_record);
    while (out->total != 100000 && read_record(z, buf, r) && r.tid >= 0) {
        const int in = in_library(r);
        if (in < 0) return no_rg(r);
        out->in_lib += (uint64_t)in;
        ++out->total;
    }
    if (z.crc_failed()) return fail(SVT_ERR_INVALID, z.crc_error());
    if (z.failed()) return fail(SVT_ERR_INVALID, "corrupt BGZF block in " + bam->path);
    out->n_hist = hist_keys.size();
    out->hist_keys = static_cast<int64_t*>(std::malloc(std::max<size_t>(hist_keys.size(), 1) * sizeof(int64_t)));
    out->hist_counts = static_cast<uint64_t*>(std::malloc(std::max<size_t>(hist_keys.size(), 1) * sizeof(uint64_t)));
    if (!out->hist_keys || !out->hist_counts) {
        svt_library_scan_free(out);
        return fail(SVT_ERR_NOMEM, "out of host memory");
    }
    if (!hist_keys.empty()) {
        std::memcpy(out->hist_keys, hist_keys.data(), hist_keys.size() * sizeof(int64_t));
        std::memcpy(out->hist_counts, hist_counts.data(), hist_counts.size() * sizeof(uint64_t));
    }
    return SVT_OK;
}

int svt_bam_scan_library(const svt_bam* bam, uint32_t n_read_groups, const char* const* read_groups, int64_t num_samp, svt_library_scan* out)
{
    return guarded([&] {
        svt::VerifyScope verify_scope(bam);
        return svt_bam_scan_library_impl(bam, n_read_groups, read_groups, num_samp, out);
    });
}

void svt_library_scan_free(svt_library_scan* s)
{
    if (!s) return;
    std::free(s->hist_keys);
    std::free(s->hist_counts);
    s->hist_keys = nullptr;
    s->hist_counts = nullptr;
    s->n_hist = 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------
// the library scans of a whole file in one segmented walk (svt_library_walk.h, svt_library_arena.h)
// ------------------------------------------------------------------------------------------

namespace svt {
namespace lw {

namespace {

thread_local uint32_t g_overflow_limit = 0;              // svt_library_scan_overflow_limit: 0 = the capacity

constexpr uint64_t kDefaultRoundBytes = 64ull << 20, kMinRoundBytes = 256ull << 10, kMaxRoundBytes = 1ull << 30;

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The rounds of one call.  A round takes whole BGZF members from the block of its first record until they inflate to round_bytes,
// and ends at the last segment start in them; the blocks behind that start are the next round's.  Where one segment alone is
// longer than a round (the unindexed tail of a file) the round is that segment's head, cut open at the arena's end, and the next
// round starts at the record the count pass stopped in front of.
struct Planner {
    const svt_bam* bam;
    const uint64_t round_bytes;
    std::vector<uint64_t> cuts;                          // the index's record starts behind first_record, ascending and distinct
    size_t next_cut = 0;
    uint64_t start;                                      // virtual offset of the next round's first record
    uint32_t seg_index = 0;
    bool stream_end = false;                             // the round planned last reaches the end of the data
    std::vector<uint64_t> member_coff;                   // of the round planned last: its members' file offsets, and the one behind
    bool open = false;                                   // ... and whether it is one open segment

    Planner(const svt_bam* b, uint64_t rb) : bam(b), round_bytes(rb), start(b->first_record)
    {
        b->index.record_starts(b->first_record, cuts);       // (BAI: the linear offsets; CSI: loffsets and chunk begins)
    }

    uint32_t plan(Round& r)
    {
        r = Round();
        r.set.file = bam->file.data;
        r.set.file_size = bam->file.size;
        member_coff.clear();
        open = false;
        const uint64_t file_size = bam->file.size;
        struct Bound { uint64_t at; size_t members, cut; };  // arena offset, members in front of it, which cut
        std::vector<Bound> bounds;
        while (next_cut < cuts.size() && cuts[next_cut] <= start) ++next_cut;
        size_t ci = next_cut;
        uint64_t coff = start >> 16, dst = 0;
        const uint32_t first_uoff = (uint32_t)(start & 0xFFFF);
        std::vector<uint64_t> ends;                      // file offset behind member k
        const uint64_t span_off = coff;
        bool eof = false;
        for (;;) {
            if (coff + 18 > file_size) { eof = true; break; }     // (where the reader's Bgzf ends the data)
            uint64_t src = 0, next = 0;
            uint32_t clen = 0, isize = 0;
            if (!inf::member_at(bam->file.data, file_size, coff, src, clen, isize, next)) return LW_MEMBER;
            if (r.set.members.empty() && first_uoff > isize) return LW_INDEX;
            if (ci < cuts.size() && (cuts[ci] >> 16) < coff) return LW_INDEX;      // an offset into a block the chain passed by
            for (; ci < cuts.size() && (cuts[ci] >> 16) == coff; ++ci) {
                const uint32_t u = (uint32_t)(cuts[ci] & 0xFFFF);
                if (u > isize) return LW_INDEX;
                bounds.push_back(Bound{dst + u, r.set.members.size() + (u ? 1u : 0u), ci});
            }
            r.set.members.push_back(inf::Member{src - span_off, clen, isize, dst});
            member_coff.push_back(coff);
            ends.push_back(next);
            dst += isize;
            coff = next;
            if (dst >= round_bytes) break;
        }
        if (eof && ci < cuts.size()) return LW_INDEX;                              // offsets behind the end of the data
        stream_end = eof;
        uint64_t begin = first_uoff;
        size_t n_bounds = bounds.size();
        if (!eof && n_bounds) {                                                     // ends at the last segment start
            const Bound& last = bounds.back();
            r.set.members.resize(last.members);
            member_coff.resize(last.members);
            ends.resize(last.members);
            start = cuts[last.cut];
            next_cut = last.cut + 1;
        }
        r.set.arena_bytes = r.set.members.empty() ? 0 : r.set.members.back().dst + r.set.members.back().isize;
        r.set.compressed_bytes = r.set.members.empty() ? 0 : ends.back() - span_off;
        r.set.spans.assign(1, bgzf::MemberSet::Span{span_off, r.set.compressed_bytes, 0});
        member_coff.push_back(r.set.members.empty() ? span_off : ends.back());
        if (begin > r.set.arena_bytes) return LW_INDEX;
        for (size_t k = 0; k < n_bounds; ++k) {
            if (bounds[k].at < begin || bounds[k].at > r.set.arena_bytes) return LW_INDEX;
            r.segments.push_back(Segment{(uint32_t)begin, (uint32_t)bounds[k].at, seg_index++, 0});
            begin = bounds[k].at;
        }
        if (eof) r.segments.push_back(Segment{(uint32_t)begin, (uint32_t)r.set.arena_bytes, seg_index++, 0});
        else if (!n_bounds) {
            r.segments.push_back(Segment{(uint32_t)begin, (uint32_t)r.set.arena_bytes, seg_index++, 1});
            open = true;
        }
        return LW_OK;
    }
    // behind an open round: the next one starts where its count pass stopped
    uint32_t advance(const Round& r, const SegCount& last)
    {
        if (!open) return LW_OK;
        if (last.stop <= r.segments.back().begin || last.stop > r.set.arena_bytes) return LW_RECORD;   // (a round holds a whole record at least)
        size_t k = r.set.members.size();
        while (k > 0 && r.set.members[k - 1].dst > last.stop) --k;                     // the last member that begins at or in front of it
        if (k == 0) return LW_RECORD;
        const inf::Member& m = r.set.members[k - 1];
        if (last.stop - m.dst >= m.isize) start = member_coff[k] << 16;            // (behind its bytes: the next block's first)
        else start = (member_coff[k - 1] << 16) | (last.stop - m.dst);
        return LW_OK;
    }
};

// the walk with one lane over tables on the heap
struct HostBackend : Backend {
    std::vector<uint8_t> arena;
    std::vector<ew::NameRef> rgs;
    std::vector<uint8_t> blob;
    HostTables T;
    std::vector<Overflow> overflow;
    uint32_t overflow_cap = 0;
    std::unique_ptr<Scratch> S{new Scratch()};
    Params params(const std::vector<Segment>& segments)
    {
        Params P{};
        P.arena = arena.data();
        P.arena_len = arena.size() - 8;
        P.segments = segments.data();
        P.rgs = rgs.data();
        P.blob = blob.data();
        P.n_rgs = (uint32_t)rgs.size();
        P.n_libs = T.n_libs;
        P.T = Tables{T.dense_count.data(), T.dense_first.data(), T.read_length.data(), T.in_lib.data(), overflow.data(), &T.overflow_n, overflow_cap};
        return P;
    }
    int begin(const std::vector<ew::NameRef>& rgs_, const std::vector<uint8_t>& blob_, uint32_t n_libs, uint32_t cap) override
    {
        rgs = rgs_;
        blob = blob_;
        T.n_libs = n_libs;
        T.dense_count.assign((size_t)n_libs * kDenseKeys, 0);
        T.dense_first.assign((size_t)n_libs * kDenseKeys, ~0ull);
        T.read_length.assign(kMaxLibs, 0);
        T.in_lib.assign(kMaxLibs, 0);
        overflow.assign(std::max<uint32_t>(cap, 1), Overflow{0, 0, 0});
        overflow_cap = cap;
        return SVT_OK;
    }
    int load(const Round& r, std::vector<uint32_t>& status, svt_library_scan_stats& S_) override
    {
        const auto t0 = std::chrono::steady_clock::now();
        arena.assign(r.set.arena_bytes + 8, 0);
        bgzf::inflate_members_host(r.set, arena.data(), 1, bgzf::Decoder::one_source, bgzf::Crc::library, r.verify, status);
        S_.inflate_s += seconds_since(t0);
        return SVT_OK;
    }
    int count(const std::vector<Segment>& segments, std::vector<SegCount>& counts) override
    {
        counts.assign(segments.size(), SegCount{});
        Params P = params(segments);
        P.counts = counts.data();
        P.n_segments = (uint32_t)segments.size();
        for (uint32_t si = 0; si < P.n_segments; ++si) walk_segment<HostCtx, false>(P, si, *S);
        return SVT_OK;
    }
    int accumulate(const std::vector<Segment>& segments, const std::vector<SegCaps>& caps) override
    {
        Params P = params(segments);
        P.caps = caps.data();
        P.n_segments = (uint32_t)caps.size();
        for (uint32_t si = 0; si < P.n_segments; ++si) walk_segment<HostCtx, true>(P, si, *S);
        return SVT_OK;
    }
    int finish(HostTables& out) override
    {
        T.overflow.assign(overflow.begin(), overflow.begin() + std::min(T.overflow_n, overflow_cap));
        out = std::move(T);
        return SVT_OK;
    }
};

void free_scans(svt_library_scan* out, uint32_t n)
{
    for (uint32_t l = 0; l < n; ++l) svt_library_scan_free(out + l);
}

}  // namespace

int scan_libraries(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts, const char* const* read_groups, int64_t num_samp,
                   uint64_t round_bytes, Backend& backend, svt_library_scan* out, svt_library_scan_stats* stats)
{
    svt_library_scan_stats local{};
    svt_library_scan_stats& S = stats ? *stats : local;
    S = svt_library_scan_stats{};
    if (!bam || !out || (n_libs && !rg_counts)) return fail(SVT_ERR_INVALID, "null argument");
    uint64_t n_rgs = 0;
    for (uint32_t l = 0; l < n_libs; ++l) { out[l] = svt_library_scan{}; n_rgs += rg_counts[l]; }
    if (n_rgs && !read_groups) return fail(SVT_ERR_INVALID, "null argument");
    if (round_bytes == 0) round_bytes = kDefaultRoundBytes;
    round_bytes = std::min(std::max(round_bytes, kMinRoundBytes), kMaxRoundBytes);

    // svt_bam_scan_library per library: the answer for everything outside the envelope, with its own errors
    auto host_answer = [&](uint32_t reason) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        S.host_reason = reason;
        free_scans(out, n_libs);
        uint64_t at = 0;
        for (uint32_t l = 0; l < n_libs; ++l) {
            const int rc = svt_bam_scan_library_impl(bam, rg_counts[l], read_groups + at, num_samp, out + l);
            if (rc != SVT_OK) { free_scans(out, n_libs); return rc; }
            at += rg_counts[l];
        }
        S.host_scan_s = seconds_since(t0);
        return SVT_OK;
    };
    if (!bam->has_index()) return host_answer(LW_NO_INDEX);
    if (n_libs == 0) return SVT_OK;
    if (n_libs > kMaxLibs || n_rgs > kMaxReadGroups) return host_answer(LW_TABLES);
    std::vector<ew::NameRef> rgs;
    std::vector<uint8_t> blob;
    {
        std::set<std::string> seen;
        uint64_t at = 0;
        for (uint32_t l = 0; l < n_libs; ++l)
            for (uint32_t k = 0; k < rg_counts[l]; ++k, ++at) {
                if (!read_groups[at]) return fail(SVT_ERR_INVALID, "null argument");
                const std::string id(read_groups[at]);
                if (!seen.insert(id).second) return host_answer(LW_TABLES);     // (a read group of two libraries: each host scan counts it)
                rgs.push_back(ew::NameRef{(uint32_t)blob.size(), (uint32_t)id.size(), (int32_t)l});
                blob.insert(blob.end(), id.begin(), id.end());
            }
        blob.resize(blob.size() + 8, 0);
        rgs.push_back(ew::NameRef{0, 0xFFFFFFFFu, -1});                         // (never an empty array; no value has this length)
    }
    const uint32_t overflow_cap = g_overflow_limit && g_overflow_limit < kOverflowCap ? g_overflow_limit : kOverflowCap;

    auto t0 = std::chrono::steady_clock::now();
    Planner planner(bam, round_bytes);
    S.index_s += seconds_since(t0);
    if (const int rc = backend.begin(rgs, blob, n_libs, overflow_cap)) return rc;

    uint64_t records_seen = 0, reads_seen[kMaxLibs] = {0}, qual_seen[kMaxLibs] = {0};
    Round r;
    std::vector<uint32_t> member_status;
    std::vector<SegCount> counts;
    std::vector<SegCaps> caps;
    for (;;) {
        t0 = std::chrono::steady_clock::now();
        if (const uint32_t reason = planner.plan(r)) return host_answer(reason);
        r.verify = bam_verify(bam);
        S.index_s += seconds_since(t0);
        ++S.rounds;
        S.segments += r.segments.size();
        S.members_inflated += r.set.members.size();
        S.compressed_bytes += r.set.compressed_bytes;
        S.inflated_bytes += r.set.arena_bytes;
        if (const int rc = backend.load(r, member_status, S)) return rc;
        for (uint32_t st : member_status)
            if (st != inf::INF_OK) return host_answer(LW_MEMBER);
        t0 = std::chrono::steady_clock::now();
        if (const int rc = backend.count(r.segments, counts)) return rc;
        S.count_s += seconds_since(t0);
        // the prefix sums in file order -> how much of every segment lies in front of each of the stops
        caps.clear();
        bool unplaced = false;
        for (size_t i = 0; i < r.segments.size() && !unplaced; ++i) {
            const SegCount& c = counts[i];
            if (c.status != LW_OK) return host_answer(c.status < LW_N_REASONS ? c.status : (uint32_t)LW_RECORD);
            SegCaps cp{};
            auto room = [](uint64_t stop, uint64_t seen, uint32_t have) { return (uint32_t)std::min<uint64_t>(have, stop > seen ? stop - seen : 0); };
            cp.records = room(kPrevalenceRecords, records_seen, c.n_records);
            cp.any = cp.records;
            for (uint32_t l = 0; l < n_libs; ++l) {
                cp.reads[l] = room(kReadLengthReads, reads_seen[l], c.reads[l]);
                cp.qual[l] = num_samp > 0 ? room((uint64_t)num_samp, qual_seen[l], c.qual[l]) : c.qual[l];   // (-n 0: the whole file)
                cp.any |= cp.reads[l] | cp.qual[l];
                reads_seen[l] += c.reads[l];
                qual_seen[l] += c.qual[l];
            }
            records_seen += c.n_records;
            S.records_walked += c.n_records;
            caps.push_back(cp);
            unplaced = c.unplaced != 0;
        }
        t0 = std::chrono::steady_clock::now();
        if (const int rc = backend.accumulate(r.segments, caps)) return rc;
        S.accumulate_s += seconds_since(t0);
        if (unplaced || planner.stream_end) break;
        bool all = records_seen >= kPrevalenceRecords;
        for (uint32_t l = 0; l < n_libs && all; ++l) all = reads_seen[l] >= kReadLengthReads && num_samp > 0 && qual_seen[l] >= (uint64_t)num_samp;
        if (all) break;
        if (const uint32_t reason = planner.advance(r, counts.back())) return host_answer(reason);
    }

    t0 = std::chrono::steady_clock::now();
    HostTables T;
    if (const int rc = backend.finish(T)) return rc;
    S.overflow_entries = T.overflow_n;
    if (T.overflow_n > overflow_cap) return host_answer(LW_OVERFLOW);
    // keys in the order of their first occurrence: the order of the reference's Counter
    struct Key { uint64_t first; int64_t key; uint64_t count; };
    std::sort(T.overflow.begin(), T.overflow.end(), [](const Overflow& a, const Overflow& b) {
        return a.lib != b.lib ? a.lib < b.lib : a.key != b.key ? a.key < b.key : a.ordinal < b.ordinal;
    });
    size_t ov = 0;
    for (uint32_t l = 0; l < n_libs; ++l) {
        std::vector<Key> keys;
        for (uint32_t k = 1; k < kDenseKeys; ++k) {
            const size_t slot = (size_t)l * kDenseKeys + k;
            if (T.dense_count[slot]) keys.push_back(Key{T.dense_first[slot], (int64_t)k, T.dense_count[slot]});
        }
        while (ov < T.overflow.size() && T.overflow[ov].lib == l) {
            size_t e = ov;
            while (e < T.overflow.size() && T.overflow[e].lib == l && T.overflow[e].key == T.overflow[ov].key) ++e;
            keys.push_back(Key{T.overflow[ov].ordinal, (int64_t)T.overflow[ov].key, (uint64_t)(e - ov)});
            ov = e;
        }
        std::sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.first < b.first; });
        svt_library_scan& o = out[l];
        o.read_length = (int64_t)T.read_length[l];
        o.in_lib = T.in_lib[l];
        o.total = std::min<uint64_t>(records_seen, kPrevalenceRecords);
        o.n_hist = keys.size();
        o.hist_keys = static_cast<int64_t*>(std::malloc(std::max<size_t>(keys.size(), 1) * sizeof(int64_t)));
        o.hist_counts = static_cast<uint64_t*>(std::malloc(std::max<size_t>(keys.size(), 1) * sizeof(uint64_t)));
        if (!o.hist_keys || !o.hist_counts) { free_scans(out, n_libs); return fail(SVT_ERR_NOMEM, "out of host memory"); }
        for (size_t k = 0; k < keys.size(); ++k) { o.hist_keys[k] = keys[k].key; o.hist_counts[k] = keys[k].count; }
    }
    S.merge_s = seconds_since(t0);
    return SVT_OK;
}

}  // namespace lw
}  // namespace svt

extern "C" {

uint32_t svt_library_scan_capacity(int which)
{
    switch (which) {
    case SVT_LIBSCAN_CAP_LIBRARIES: return svt::lw::kMaxLibs;
    case SVT_LIBSCAN_CAP_READ_GROUPS: return svt::lw::kMaxReadGroups;
    case SVT_LIBSCAN_CAP_DENSE_KEYS: return svt::lw::kDenseKeys;
    case SVT_LIBSCAN_CAP_OVERFLOW: return svt::lw::kOverflowCap;
    case SVT_LIBSCAN_CAP_RECORD: return svt::lw::kMaxRecord;
    case SVT_LIBSCAN_CAP_ROUND_BYTES: return (uint32_t)svt::lw::kDefaultRoundBytes;
    default: return 0;
    }
}

void svt_library_scan_overflow_limit(uint32_t entries) { svt::lw::g_overflow_limit = entries; }

int svt_bam_scan_libraries_walk_host(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts, const char* const* read_groups,
                                     int64_t num_samp, uint64_t round_bytes, svt_library_scan* out, svt_library_scan_stats* stats)
{
    return guarded([&] {
        svt::VerifyScope verify_scope(bam);
        svt::lw::HostBackend backend;
        return svt::lw::scan_libraries(bam, n_libs, rg_counts, read_groups, num_samp, round_bytes, backend, out, stats);
    });
}

}  // extern "C"

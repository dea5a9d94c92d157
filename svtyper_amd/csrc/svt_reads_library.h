// svt_reads_library.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the scans
// of one library (svt_bam_scan_library) and the library scans of a whole file in one segmented walk (svt_library_walk.h,
// svt_library_arena.h): lw::Planner, HostBackend, scan_libraries.  Needs: Bgzf, inflate_members_host (svt_bgzf_reader.h), svt_bam,
// VerifyScope (svt_reads_handle.h), Record, read_group, read_record (svt_reads_records.h).
extern "C" {

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

namespace svt {
namespace lw {

namespace {

thread_local uint32_t g_overflow_limit = 0;              // svt_library_scan_overflow_limit: 0 = the capacity

constexpr uint64_t kDefaultRoundBytes = 64ull << 20, kMinRoundBytes = 256ull << 10, kMaxRoundBytes = 1ull << 30;

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

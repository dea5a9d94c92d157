// svt_reads_arena.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the arena
// of svt_evidence_walk.h and the host recomputation of single units (svt_evidence_arena.h): one planner, its host and open routes,
// host_units.  Needs: Bgzf, SharedBlocks (svt_bgzf_reader.h), svt_bam (svt_reads_handle.h), next_record, fetch_chunks
// (svt_reads_records.h), UnitReader (svt_reads_fragments.h).
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
    out.build_s = svt::seconds_since(t_begin);
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
    plan.index_s = out.build_s = svt::seconds_since(t_begin);
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
    const RgLibraries rg_lib = rg_library_map(*args);
    std::vector<std::vector<svt_record>> per(m);
    const unsigned nt = arena_threads(args, m);
    const std::unique_ptr<SharedBlocks> shared_blocks(new SharedBlocks());
    std::atomic<size_t> next(0);
    std::mutex err_lock;
    size_t err_at = m;                                                // the first unit (in the units' order) that failed
    int err_rc = SVT_OK;
    std::string err_text;
    run_threads(nt, [&](unsigned) {
        UnitReader R(bam, args, geometry, rg_lib, shared_blocks.get());
        for (;;) {
            const size_t k = next.fetch_add(1);
            if (k >= m) return;
            std::string err;
            const int rc = R.ok() ? R.evidence(ids[k], err) : SVT_ERR_NOMEM;
            if (rc != SVT_OK) {
                std::lock_guard<std::mutex> g(err_lock);
                if (k < err_at) { err_at = k; err_rc = rc; err_text = R.ok() ? err : "cannot set up the inflate state"; }
                continue;
            }
            per[k] = R.unit.recs;
            skipped[k] = R.unit.skipped ? 1 : 0;
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

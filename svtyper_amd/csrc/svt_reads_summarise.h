// svt_reads_summarise.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header):
// svt_bam_summarise and svt_bam_evidence -- units on worker threads, gathered into flat arrays -- and their frees.  Needs:
// UnitReader (svt_reads_fragments.h), BufferPool, SummaryArena (svt_reads_pool.h).
extern "C" {

static std::atomic<double> g_cpu_s_per_unit{0.0};   // CPU seconds per unit of the last svt_bam_summarise / svt_bam_evidence call on any file

struct UnitSpan {                      // where a finished unit's summaries (or evidence records) wait for the gather
    const void* data = nullptr;
    uint64_t count = 0;
    bool skipped = false;
};

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
    const RgLibraries rg_lib = rg_library_map(*args);

    const bool trace = std::getenv("SVT_TRACE") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (trace)
            std::fprintf(stderr, "[svt_bam_summarise] %-10s %8.1f ms\n", what, svt::seconds_since(t_begin) * 1e3);
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
        UnitReader R(bam, args, geometry, rg_lib, shared_blocks.get());
        UnitOut& unit = R.unit;
        struct Report {
            WorkerStat& st; Bgzf& z; std::chrono::steady_clock::time_point t0; double cpu0;
            ~Report() { st.cpu_s = thread_cpu_seconds() - cpu0; st.busy_s = svt::seconds_since(t0); st.inflate_s = z.inflate_s; st.inflated = z.n_inflated; st.shared = z.n_shared_hits; st.ahead = z.n_ahead; }
        } report{stats[t], R.z, w_begin, thread_cpu_seconds()};
        arenas[t].reset(new SummaryArena());
        if (!R.ok()) {
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
                // (geometry: the predicates of the device stage, here: 16 bytes per fragment leave the reader)
                int rc = geometry ? R.evidence(u, err) : R.summaries(u, err);
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

}  // extern "C"

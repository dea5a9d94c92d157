// svt_reads_walk.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// one-source walk (svt_evidence_walk.h) on the host, its dump (svt_dump_rules.h), their entry points, svt_evidence_walk_capacity. 
// Needs: build_arena, build_arena_open, arena_threads (svt_reads_arena.h), svt_evidence_free (svt_reads_summarise.h).
extern "C" {

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
    dump->dump_s = svt::seconds_since(t0);
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

// What the three entry points differ in.  `dump` (svt_bam_evidence_dump_walk_host): the walk also leaves its source rows, and the dump
// rules run over them and `verdicts`
struct HostWalkOptions { bool open_ranges; uint32_t* kept_reads; const uint8_t* verdicts; uint64_t n_verdicts; svt_evidence_dump* dump; };

static int svt_bam_evidence_walk_host_impl(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                           svt_evidence* out, uint8_t* out_of_envelope, const HostWalkOptions& opt)
{
    svt_evidence_dump* const dump = opt.dump;
    if (!out || !out_of_envelope) return fail(SVT_ERR_INVALID, "null argument");
    svt::VerifyScope verify_scope(bam);
    out->rec_offset = nullptr;
    out->records = nullptr;
    out->skipped = nullptr;
    if (dump) *dump = svt_evidence_dump{};
    svt::ew::Arena arena;
    if (opt.open_ranges) {
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
            auto walk = [&](auto& scratch, const auto& tables) {              // with source rows (kSrc) for a dump
                if (dump) svt::ew::walk_unit<svt::ew::HostCtx, std::remove_reference_t<decltype(scratch)>, true>(P, u, scratch, tables, rows.data(), src_rows.data());
                else svt::ew::walk_unit<svt::ew::HostCtx>(P, u, scratch, tables, rows.data());
            };
            walk(*S, S->tables());
            uint32_t st = S->status, n_reads = S->n_reads, n_rows = S->n_rows;
            if (svt::ew::deep_tier_unit(st, n_reads)) {
                if (!D) {
                    D.reset(new svt::ew::DeepScratch());
                    slice.reset(new uint64_t[svt::ew::kDeepSliceBytes / sizeof(uint64_t)]);
                    rows.resize(svt::ew::kMaxReadsDeep);
                    if (dump) src_rows.resize(svt::ew::kMaxReadsDeep);
                }
                walk(*D, svt::ew::deep_tables(reinterpret_cast<uint8_t*>(slice.get())));
                st = D->status; n_reads = D->n_reads; n_rows = D->n_rows;
            }
            status[u] = st;
            if (opt.kept_reads) opt.kept_reads[u] = n_reads;
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
        if (opt.n_verdicts != off || (off && !opt.verdicts)) {
            svt_evidence_free(out);
            return fail(SVT_ERR_INVALID, "svt_bam_evidence_dump_walk_host: one verdict byte per record of svt_bam_evidence_walk_host on the same arguments");
        }
        if (const int rc = dump_units_host(arena, src, status, out->rec_offset, opt.verdicts, dump)) {
            svt_evidence_free(out);
            return rc;
        }
    }
    return SVT_OK;
}

int svt_bam_evidence_dump_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, const uint8_t* verdicts,
                                    uint64_t n_verdicts, svt_evidence* out, uint8_t* out_of_envelope, svt_evidence_dump* dump)
{
    return guarded([&] {
        if (!dump) return fail(SVT_ERR_INVALID, "null argument");
        return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, HostWalkOptions{false, nullptr, verdicts, n_verdicts, dump});
    });
}

int svt_bam_evidence_walk_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out,
                               uint8_t* out_of_envelope, uint32_t* kept_reads)
{
    return guarded([&] { return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, HostWalkOptions{false, kept_reads, nullptr, 0, nullptr}); });
}

int svt_bam_evidence_walk_open_host(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry, svt_evidence* out,
                                    uint8_t* out_of_envelope, uint32_t* kept_reads)
{
    return guarded([&] { return svt_bam_evidence_walk_host_impl(bam, args, geometry, out, out_of_envelope, HostWalkOptions{true, kept_reads, nullptr, 0, nullptr}); });
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

}  // extern "C"

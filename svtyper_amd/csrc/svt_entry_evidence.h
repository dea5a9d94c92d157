// svt_entry_evidence.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// C ABI: svt_bam_evidence_device, svt_bam_evidence_device_inflate (include/svtyper_reads.h) and the read-back of a resident
// batch's records for the parity tests.  (Device inflate of the arena's members is svt_entry_inflate.h.)

// the deep tier's figures of this thread's last device-reader call (svt_evidence_device_deep_stats)
static thread_local svt_evidence_deep_stats g_deep_stats{};

// Who inflates the BGZF blocks of a device-reader call
struct EvidenceRoute {
    svt_evidence_inflate_stats* inflate_stats = nullptr;   // null: the host (svt_bam_evidence_device); else svt_inflate_kernel, into HBM
    bool count_host_blocks = false;                        // device inflate only: build the host route's arena too, for blocks_host_route
    svt_evidence_dump* dump = nullptr;                     // svt_bam_evidence_device_dump: source rows from the write pass, dump_pass() behind the batch
    bool device_inflate() const { return inflate_stats != nullptr; }
};

// One call of a device reader: its stream, its device buffers, the kernels' arguments and what one step leaves for the next.
// Destruction order (CallStream, svt_batch_state.h): ~EvidenceCall drains the stream, then the buffers are freed or go back to
// their pools, then the stream is returned.
struct EvidenceCall : CallStream {
    const svt_bam* const bam;
    const svt_summarise_args* const args;
    const svt_evidence_params* const geometry;
    const svt_evidence_batch* const header;
    const int device;
    const unsigned flags;
    const EvidenceRoute route;
    svt_evidence_device_stats& S;
    svt_evidence_deep_stats& DS = g_deep_stats;
    const uint64_t n = args->n_units;
    Pooled d_arena{device}, d_records{device}, d_compressed{device};
    DeviceInflate inflate{device};                           // inflate = "device": the members of `plan`
    DevScratch d_ranges, d_units, d_windows, d_bps, d_rgs, d_refs, d_blob, d_flank, d_status, d_rows, d_reads, d_off, d_src, d_src_off, d_dst_off;
    DevScratch d_deep_unit, d_deep_status, d_deep_rows, d_deep_workspace;   // only a call with deep units allocates these
    DevScratch d_src_rows, d_verdicts, d_unit_host, d_slot_len, d_slot_state, d_slot_off, d_unit_bytes, d_unit_reads, d_unit_outside, d_unit_offset, d_dump_error;   // only a dump call
    Pooled d_dump_bytes{device};

    ew::Arena arena;
    ew::OpenPlan plan;
    EvidenceArgs a{};
    EvidenceDeepArgs da{};
    static constexpr size_t kLds = sizeof(ew::UnitScratch);
    std::vector<uint32_t> status, rows, reads;               // per unit, from the count passes
    std::vector<uint32_t> deep_unit;
    uint32_t n_deep = 0, deep_grid = 0;
    std::vector<uint64_t> host_ids, host_counts;             // the units outside the envelope, by the reader itself
    std::vector<svt_record> host_records;
    std::vector<uint8_t> host_skipped;
    std::vector<uint64_t> rec_offset;
    std::vector<svt_unit> units;
    uint64_t n_rec = 0;

    EvidenceCall(const svt_bam* bam_, const svt_summarise_args* args_, const svt_evidence_params* geometry_, const svt_evidence_batch* header_,
                 int device_, unsigned flags_, EvidenceRoute route_, svt_evidence_device_stats& S_)
        : bam(bam_), args(args_), geometry(geometry_), header(header_), device(device_), flags(flags_), route(route_), S(S_) {}
    ~EvidenceCall() { drain(); }

    // host: BAI lookup, and either inflate + arena or the arena's layout from BGZF headers
    int build_arena()
    {
        if (route.device_inflate()) {
            svt_evidence_inflate_stats& I = *route.inflate_stats;
            I = svt_evidence_inflate_stats{};
            if (route.count_host_blocks) {
                ew::Arena host_route;
                SVT_TRY(ew::build_arena(bam, args, geometry, host_route));
                I.blocks_host_route = host_route.blocks;
            }
            SVT_TRY(ew::build_arena_open(bam, args, geometry, arena, plan));
            I.host_index_s = plan.index_s;
            I.blocks_inflated = plan.set.members.size();
            I.compressed_bytes = plan.set.compressed_bytes;
            I.inflated_bytes = plan.set.arena_bytes;
        } else SVT_TRY(ew::build_arena(bam, args, geometry, arena));
        S.host_arena_s = arena.build_s;
        S.reads_walked = arena.records_in_ranges;
        return SVT_OK;
    }
    // the arena -- its bytes, or the compressed members and the inflate kernel --, the ranges, units, names and flanks; the buffers
    // of the count pass
    int upload_inputs()
    {
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<double> flank(geometry->lib_flank, geometry->lib_flank + geometry->n_libs);
        {
            Stager st(s);
            SVT_TRY(d_arena.get(arena.bytes.size()));
            if (route.device_inflate()) {
                // the compressed members from the mapping, the inflate kernel, the statuses; a unit over a failed member is the host's
                svt_evidence_inflate_stats& I = *route.inflate_stats;
                SVT_TRY(d_compressed.get(plan.set.compressed_bytes + 8));
                SVT_TRY(inflate.upload(plan.set, d_compressed.p, st, bam_verify(bam)));   // (verify: the expected CRC-32s go up with the member table)
                SVT_TRY(st.finish());
                I.compressed_upload_s = seconds_since(t0);
                const auto t_kernel = std::chrono::steady_clock::now();
                std::vector<uint32_t> member_status;
                SVT_TRY(inflate.run(d_compressed.p, d_arena.p, s, member_status));
                I.inflate_kernel_s = seconds_since(t_kernel);
                I.blocks_failed = ew::apply_member_status(plan, member_status, arena);
            } else SVT_TRY(st.copy(d_arena.p, arena.bytes.data(), arena.bytes.size()));
            SVT_TRY(upload(d_ranges, arena.ranges, st));
            SVT_TRY(upload(d_units, arena.units, st));
            SVT_TRY(d_windows.alloc(n * sizeof(svt_fetch_unit)));
            SVT_TRY(st.copy(d_windows.p, args->windows, n * sizeof(svt_fetch_unit)));
            SVT_TRY(d_bps.alloc(n * sizeof(svt_breakpoint)));
            SVT_TRY(st.copy(d_bps.p, args->breakpoints, n * sizeof(svt_breakpoint)));
            SVT_TRY(upload(d_rgs, arena.rgs, st));
            SVT_TRY(upload(d_refs, arena.refs, st));
            SVT_TRY(upload(d_blob, arena.blob, st));
            SVT_TRY(upload(d_flank, flank, st));
            SVT_TRY(st.finish());
            S.bytes_uploaded = (route.device_inflate() ? plan.set.compressed_bytes + plan.set.members.size() * sizeof(inf::Member) : arena.bytes.size()) + arena.ranges.size() * sizeof(ew::Range) + n * (sizeof(ew::UnitRanges) + sizeof(svt_fetch_unit) + sizeof(svt_breakpoint)) + arena.blob.size();
        }
        SVT_TRY(d_status.alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_rows.alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_reads.alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_off.alloc((n + 1) * sizeof(uint64_t)));
        HIP_TRY(hipStreamSynchronize(s));
        S.upload_s = seconds_since(t0);
        return SVT_OK;
    }
    // the kernels' arguments over the uploaded buffers
    int bind_arguments()
    {
        a.P = arena.params(args, geometry);
        a.P.arena = static_cast<const uint8_t*>(d_arena.p);
        a.P.ranges = d_ranges.as<ew::Range>();
        a.P.units = d_units.as<ew::UnitRanges>();
        a.P.windows = d_windows.as<svt_fetch_unit>();
        a.P.bps = d_bps.as<svt_breakpoint>();
        a.P.rgs = d_rgs.as<ew::NameRef>();
        a.P.refs = d_refs.as<ew::NameRef>();
        a.P.blob = d_blob.as<uint8_t>();
        a.P.lib_flank = d_flank.as<double>();
        a.n_units = (uint32_t)n;
        a.status = d_status.as<uint32_t>();
        a.n_rows = d_rows.as<uint32_t>();
        a.n_reads = d_reads.as<uint32_t>();
        a.rec_offset = d_off.as<uint64_t>();
        a.records = nullptr;
        static_assert(sizeof(ew::UnitScratch) <= 80 * 1024, "two workgroups of the evidence kernel per CU");
        static_assert(sizeof(ew::DeepScratch) <= 64 * 1024, "the deep kernel's static LDS");
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&svt_evidence_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&svt_evidence_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
        return SVT_OK;
    }
    // launch 1: status and rows per unit
    int count_pass()
    {
        status.resize(n);
        rows.resize(n);
        reads.resize(n);
        if (n) {
            hipLaunchKernelGGL(svt_evidence_kernel<false>, dim3((unsigned)n), dim3(kEvidenceBlock), kLds, s, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(status.data(), d_status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(rows.data(), d_rows.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(reads.data(), d_reads.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        return SVT_OK;
    }
    // launch 1b: the units the LDS tier counted beyond its table, up to the deep tier's capacity, with their tables in HBM.
    // In d_status they stay EW_READS, so the LDS tier's write pass leaves them alone; their verdicts are the deep kernel's.
    int deep_count()
    {
        for (uint64_t u = 0; u < n; ++u)
            if (ew::deep_tier_unit(status[u], reads[u])) {
                deep_unit.push_back((uint32_t)u);
                DS.reads_deep += reads[u];
            }
        n_deep = (uint32_t)deep_unit.size();
        deep_grid = std::min(n_deep, kDeepMaxSlices);
        if (!n_deep) return SVT_OK;
        const auto t_deep = std::chrono::steady_clock::now();
        std::vector<uint32_t> deep_status(n_deep), deep_rows(n_deep);
        DS.units_deep = n_deep;
        DS.workspace_bytes = (uint64_t)deep_grid * ew::kDeepSliceBytes;
        SVT_TRY(d_deep_workspace.alloc(DS.workspace_bytes));
        SVT_TRY(d_deep_status.alloc(n_deep * sizeof(uint32_t)));
        SVT_TRY(d_deep_rows.alloc(n_deep * sizeof(uint32_t)));
        {
            Stager st(s);
            SVT_TRY(upload(d_deep_unit, deep_unit, st));
            SVT_TRY(st.finish());
        }
        da.P = a.P;
        da.n_deep = n_deep;
        da.unit = d_deep_unit.as<uint32_t>();
        da.status = d_deep_status.as<uint32_t>();
        da.n_rows = d_deep_rows.as<uint32_t>();
        da.rec_offset = d_off.as<uint64_t>();
        da.records = nullptr;
        da.workspace = d_deep_workspace.as<uint8_t>();
        hipLaunchKernelGGL(svt_evidence_deep_kernel<false>, dim3(deep_grid), dim3(kEvidenceBlock), 0, s, da);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(deep_status.data(), d_deep_status.p, n_deep * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(deep_rows.data(), d_deep_rows.p, n_deep * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < n_deep; ++k) { status[deep_unit[k]] = deep_status[k]; rows[deep_unit[k]] = deep_rows[k]; }
        DS.deep_walk_s = seconds_since(t_deep);
        return SVT_OK;
    }
    // host: the units outside the envelope, by the reader itself
    int host_fallback()
    {
        for (uint64_t u = 0; u < n; ++u) {
            if (status[u] >= ew::EW_N_STATUS) return fail(SVT_ERR_INTERNAL, "svt_bam_evidence_device: unit status out of range");
            if (status[u] >= ew::EW_RANGE) {
                host_ids.push_back(u);
                ++S.units_host_by_reason[status[u]];
            }
        }
        S.units_host = host_ids.size();
        return ew::host_units(bam, args, geometry, host_ids, host_records, host_counts, host_skipped);
    }
    // rec_offset: the counts of both kinds of units in one scan
    int offset_scan(uint8_t* skipped_out)
    {
        rec_offset.assign(n + 1, 0);
        units.assign(header->units, header->units + n);
        size_t hk = 0;
        for (uint64_t u = 0; u < n; ++u) {
            uint64_t cnt = rows[u];
            bool skip = status[u] == ew::EW_SKIPPED;
            if (hk < host_ids.size() && host_ids[hk] == u) { cnt = host_counts[hk]; skip = host_skipped[hk] != 0; ++hk; }
            rec_offset[u + 1] = rec_offset[u] + cnt;
            if (skip) { units[u].flags |= SVT_UNIT_SKIP; ++S.units_skipped; }
            if (skipped_out) skipped_out[u] = skip ? 1 : 0;
        }
        n_rec = rec_offset[n];
        S.n_records = n_rec;
        if (n_rec > max_batch_records()) return fail(SVT_ERR_INVALID, "too many records in one batch (< 2^32): cut the call into fewer units");
        return SVT_OK;
    }
    // launch 2: the records, where the batch wants them; then the host's units into their places; then the deep units' records
    int write_pass()
    {
        SVT_TRY(d_records.get((n_rec + kBlockRecords) * sizeof(uint4), /*records=*/true));   // whole 128-byte blocks (kLayoutStream)
        {
            Stager st(s);
            SVT_TRY(st.copy(d_off.p, rec_offset.data(), (n + 1) * sizeof(uint64_t)));
            if (!host_ids.empty()) {
                std::vector<uint64_t> src_off(host_ids.size() + 1, 0), dst_off(host_ids.size());
                for (size_t k = 0; k < host_ids.size(); ++k) { src_off[k + 1] = src_off[k] + host_counts[k]; dst_off[k] = rec_offset[host_ids[k]]; }
                SVT_TRY(upload(d_src, host_records, st));
                SVT_TRY(upload(d_src_off, src_off, st));
                SVT_TRY(upload(d_dst_off, dst_off, st));
            }
            SVT_TRY(st.finish());
        }
        a.records = static_cast<uint4*>(d_records.p);
        if (route.dump) {                                        // a source row beside every record (all ones where a row is the host reader's)
            SVT_TRY(d_src_rows.alloc(n_rec * sizeof(ew::SrcRow)));
            if (n_rec) HIP_TRY(hipMemsetAsync(d_src_rows.p, 0xff, n_rec * sizeof(ew::SrcRow), s));
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&svt_evidence_src_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds));
        }
        if (n && route.dump) {
            hipLaunchKernelGGL(svt_evidence_src_kernel, dim3((unsigned)n), dim3(kEvidenceBlock), kLds, s, a, d_src_rows.as<ew::SrcRow>());
            HIP_TRY(hipGetLastError());
        } else if (n) {
            hipLaunchKernelGGL(svt_evidence_kernel<true>, dim3((unsigned)n), dim3(kEvidenceBlock), kLds, s, a);
            HIP_TRY(hipGetLastError());
        }
        if (!host_ids.empty()) {
            hipLaunchKernelGGL(svt_evidence_scatter_kernel, dim3((unsigned)host_ids.size()), dim3(kEvidenceBlock), 0, s, d_src.as<uint4>(),
                               d_src_off.as<uint64_t>(), d_dst_off.as<uint64_t>(), (uint32_t)host_ids.size(), static_cast<uint4*>(d_records.p));
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(s));
        if (n_deep) {                                            // (behind a sync of its own: its time is reported apart)
            const auto t_deep = std::chrono::steady_clock::now();
            da.records = static_cast<uint4*>(d_records.p);
            if (route.dump) hipLaunchKernelGGL(svt_evidence_deep_src_kernel, dim3(deep_grid), dim3(kEvidenceBlock), 0, s, da, d_src_rows.as<ew::SrcRow>());
            else hipLaunchKernelGGL(svt_evidence_deep_kernel<true>, dim3(deep_grid), dim3(kEvidenceBlock), 0, s, da);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
            DS.deep_walk_s += seconds_since(t_deep);
        }
        return SVT_OK;
    }
    // the resident batch, from the records that are already in HBM
    int make_batch(svt_batch** out)
    {
        svt_evidence_batch eb = *header;
        eb.rec_offset = rec_offset.data();
        eb.units = units.data();
        eb.records = nullptr;
        if (const char* e = evidence_error(&eb, flags, /*records_may_be_null=*/true)) return fail(SVT_ERR_INVALID, e);
        BatchOwner b;
        SVT_TRY(new_batch(&b, device, flags, kLayoutStream, n, n_rec));
        const int rc = create_stream(&eb, b.get(), d_records.p, d_records.cap);
        if (b->d_records == d_records.p) d_records.release();   // the batch owns the records now
        SVT_TRY(rc);
        *out = b.release();
        return SVT_OK;
    }
    // The evidence dump, behind the batch: svt_verdict_kernel over the new batch (its bytes stay in HBM), then the two launches of
    // svt_dump_kernel.h with the host's prefix sum between them, all on the call's stream.
    int dump_pass(svt_batch* b)
    {
        svt_evidence_dump& D = *route.dump;
        const auto t0 = std::chrono::steady_clock::now();
        D.unit_offset = static_cast<uint64_t*>(std::calloc(n + 1, sizeof(uint64_t)));
        D.unit_host = static_cast<uint8_t*>(std::calloc(std::max<uint64_t>(n, 1), 1));
        if (!D.unit_offset || !D.unit_host) return fail(SVT_ERR_NOMEM, "out of host memory");
        for (const uint64_t u : host_ids) D.unit_host[u] = 1;
        if (n == 0 || n_rec == 0) {
            D.units_host = host_ids.size();
            D.bytes = static_cast<uint8_t*>(std::malloc(1));
            D.dump_s = seconds_since(t0);
            return D.bytes ? SVT_OK : fail(SVT_ERR_NOMEM, "out of host memory");
        }
        HIP_TRY(hipStreamSynchronize(b->stream));                // (the batch's tables and offsets are up)
        SVT_TRY(d_verdicts.alloc(n_rec));
        SVT_TRY(launch_verdicts(b, d_verdicts.as<uint8_t>(), s));
        SVT_TRY(d_unit_host.alloc(n));
        SVT_TRY(d_slot_len.alloc(2 * n_rec * sizeof(uint32_t)));
        SVT_TRY(d_slot_state.alloc(2 * n_rec));
        SVT_TRY(d_slot_off.alloc(2 * n_rec * sizeof(uint32_t)));
        SVT_TRY(d_unit_bytes.alloc(n * sizeof(uint64_t)));
        SVT_TRY(d_unit_outside.alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_unit_reads.alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_unit_offset.alloc((n + 1) * sizeof(uint64_t)));
        SVT_TRY(d_dump_error.alloc(sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d_unit_host.p, D.unit_host, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_slot_len.p, 0, 2 * n_rec * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(d_slot_state.p, 0, 2 * n_rec, s));
        HIP_TRY(hipMemsetAsync(d_dump_error.p, 0, sizeof(uint32_t), s));
        DumpArgs da2{};
        da2.arena = static_cast<const uint8_t*>(d_arena.p);
        da2.arena_len = arena.bytes.size();
        da2.rows = d_src_rows.as<ew::SrcRow>();
        da2.verdicts = d_verdicts.as<uint8_t>();
        da2.rec_offset = b->d_off;
        da2.unit_host = d_unit_host.as<uint8_t>();
        da2.n_units = (uint32_t)n;
        da2.slot_len = d_slot_len.as<uint32_t>();
        da2.slot_state = d_slot_state.as<uint8_t>();
        da2.slot_off = d_slot_off.as<uint32_t>();
        da2.unit_bytes = d_unit_bytes.as<uint64_t>();
        da2.unit_outside = d_unit_outside.as<uint32_t>();
        da2.unit_reads = d_unit_reads.as<uint32_t>();
        da2.unit_offset = d_unit_offset.as<uint64_t>();
        da2.error = d_dump_error.as<uint32_t>();
        constexpr unsigned kUnitsPerWg = kDumpBlock / kWave;
        hipLaunchKernelGGL(svt_dump_size_kernel, dim3((unsigned)((n + kUnitsPerWg - 1) / kUnitsPerWg)), dim3(kDumpBlock), 0, s, da2);
        HIP_TRY(hipGetLastError());
        std::vector<uint64_t> unit_bytes(n);
        std::vector<uint32_t> unit_outside(n), unit_reads(n);
        HIP_TRY(hipMemcpyAsync(unit_bytes.data(), d_unit_bytes.p, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(unit_outside.data(), d_unit_outside.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(unit_reads.data(), d_unit_reads.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t u = 0; u < n; ++u) {
            if (unit_outside[u] && !D.unit_host[u]) { D.unit_host[u] = 1; ++D.units_outside_dump; }
            D.unit_offset[u + 1] = D.unit_offset[u] + (D.unit_host[u] ? 0 : unit_bytes[u]);
            D.units_host += D.unit_host[u];
            D.units_dumped += D.unit_offset[u + 1] != D.unit_offset[u];
            if (!D.unit_host[u]) D.n_reads += unit_reads[u];
        }
        D.n_bytes = D.unit_offset[n];
        D.bytes = static_cast<uint8_t*>(std::malloc(std::max<uint64_t>(D.n_bytes, 1)));
        if (!D.bytes) return fail(SVT_ERR_NOMEM, "out of host memory");
        if (D.n_bytes) {
            SVT_TRY(d_dump_bytes.get(D.n_bytes));
            da2.bytes = static_cast<uint8_t*>(d_dump_bytes.p);
            HIP_TRY(hipMemcpyAsync(d_unit_host.p, D.unit_host, n, hipMemcpyHostToDevice, s));      // (with the units outside the dump's envelope)
            HIP_TRY(hipMemcpyAsync(d_unit_offset.p, D.unit_offset, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(svt_dump_write_kernel, dim3((unsigned)n), dim3(kDumpBlock), 0, s, da2);
            HIP_TRY(hipGetLastError());
            uint32_t error = 0;
            HIP_TRY(hipMemcpyAsync(&error, d_dump_error.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            SVT_TRY(d2h_staged(D.bytes, d_dump_bytes.p, D.n_bytes, s));
            if (error) return fail(SVT_ERR_INTERNAL, "svt_bam_evidence_device_dump: a read does not give the bytes it was sized for");
        }
        D.dump_s = seconds_since(t0);
        return SVT_OK;
    }
};

// Both device readers: everything behind the arena -- the walk launches, the fallback, the scan, the batch -- is the same code.
static int svt_bam_evidence_device_impl(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                        const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out,
                                        uint8_t* skipped_out, svt_evidence_device_stats* stats, EvidenceRoute route)
{
    g_deep_stats = svt_evidence_deep_stats{};                // (in front of every way out: the figures are this call's, also when it fails)
    if (!bam || !args || !geometry || !header || !out) return fail(SVT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (header->n_units != args->n_units) return fail(SVT_ERR_INVALID, "svt_bam_evidence_device: header and args differ in n_units");
    if (args->n_units && !header->units) return fail(SVT_ERR_INVALID, "null unit arrays");
    if (header->n_libs != geometry->n_libs) return fail(SVT_ERR_INVALID, "svt_bam_evidence_device: header and geometry differ in n_libs");
    svt_evidence_device_stats st_local{};
    svt_evidence_device_stats& S = stats ? *stats : st_local;
    S = svt_evidence_device_stats{};
    S.n_units = args->n_units;
    VerifyScope verify_scope(bam);

    EvidenceCall c(bam, args, geometry, header, device, flags, route, S);
    SVT_TRY(c.build_arena());
    SVT_TRY(select_device(device));
    SVT_TRY(c.take());
    SVT_TRY(c.upload_inputs());                              // (S.upload_s; device inflate: its kernel too)
    SVT_TRY(c.bind_arguments());

    auto t0 = std::chrono::steady_clock::now();
    SVT_TRY(c.count_pass());
    SVT_TRY(c.deep_count());
    S.device_walk_s = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    SVT_TRY(c.host_fallback());
    S.host_fallback_s = seconds_since(t0);
    SVT_TRY(c.offset_scan(skipped_out));
    t0 = std::chrono::steady_clock::now();
    SVT_TRY(c.write_pass());
    S.device_walk_s += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    SVT_TRY(c.make_batch(out));
    S.batch_create_s = seconds_since(t0);
    if (route.dump) {
        const int rc = c.dump_pass(*out);
        if (rc != SVT_OK) {                                      // (no batch without its dump)
            c.drain();
            BatchOwner(*out).reset();
            *out = nullptr;
            svt_evidence_dump_free(route.dump);
            return rc;
        }
    }
    return SVT_OK;
}

int svt_bam_evidence_device(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                            const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out, uint8_t* skipped,
                            svt_evidence_device_stats* stats)
{
    return guarded([&] { return svt_bam_evidence_device_impl(bam, args, geometry, header, device, flags, out, skipped, stats, EvidenceRoute{}); });
}

int svt_bam_evidence_device_inflate(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                    const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out, uint8_t* skipped,
                                    svt_evidence_device_stats* stats, svt_evidence_inflate_stats* istats, int count_host_blocks)
{
    return guarded([&] {
        svt_evidence_inflate_stats local{};
        return svt_bam_evidence_device_impl(bam, args, geometry, header, device, flags, out, skipped, stats,
                                            EvidenceRoute{istats ? istats : &local, count_host_blocks != 0});
    });
}

int svt_bam_evidence_device_dump(const svt_bam* bam, const svt_summarise_args* args, const svt_evidence_params* geometry,
                                 const svt_evidence_batch* header, int device, unsigned flags, svt_batch** out, uint8_t* skipped,
                                 svt_evidence_device_stats* stats, svt_evidence_inflate_stats* istats, int count_host_blocks,
                                 int inflate_on_device, svt_evidence_dump* dump)
{
    return guarded([&] {
        if (!dump) return fail(SVT_ERR_INVALID, "null argument");
        *dump = svt_evidence_dump{};
        svt_evidence_inflate_stats local{};
        EvidenceRoute route;
        if (inflate_on_device) { route.inflate_stats = istats ? istats : &local; route.count_host_blocks = count_host_blocks != 0; }
        route.dump = dump;
        return svt_bam_evidence_device_impl(bam, args, geometry, header, device, flags, out, skipped, stats, route);
    });
}

int svt_evidence_device_deep_stats(svt_evidence_deep_stats* out)
{
    return guarded([&]() -> int {
        if (!out) return fail(SVT_ERR_INVALID, "null argument");
        *out = g_deep_stats;
        return SVT_OK;
    });
}

// the records and offsets of a resident batch of canonical records, back on the host (parity tests of the device reader):
// rec_offset holds n_units + 1 entries, records rec_offset[n_units] (pass null to fetch only the offsets)
int svt_debug_batch_records(svt_batch* b, uint64_t* rec_offset, svt_record* records)
{
    return guarded([&]() -> int {
        if (!b || !rec_offset) return fail(SVT_ERR_INVALID, "null argument");
        if (b->layout != kLayoutStream || !b->records_resident) return fail(SVT_ERR_INVALID, "canonical resident records only");
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));
        if (b->n_units == 0) { rec_offset[0] = 0; return SVT_OK; }      // (a batch without units has no offsets in HBM)
        HIP_TRY(hipMemcpy(rec_offset, b->d_off, (b->n_units + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (records && b->n_records) HIP_TRY(hipMemcpy(records, b->d_records, b->n_records * sizeof(svt_record), hipMemcpyDeviceToHost));
        return SVT_OK;
    });
}

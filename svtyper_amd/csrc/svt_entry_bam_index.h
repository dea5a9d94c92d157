// svt_entry_bam_index.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_bam_sort.h; not a stand-alone header): the CSI fold of the `-w` BAM on the device.  What is this header's: the launches
// of svt_bam_index_kernel.h over a span table that is resident already (fold_resident: the record kernel, the three-phase scan
// with the compaction in its last phase, the runs through the fold's own RadixSort (svt_entry_radix_sort.h), the loffsets, the
// per-reference rows), the check of what came down, the serialiser's call (svt_tbx_index.h: csi::serialise -- the host fold's)
// and the bytes left for svt_csi_take.  What goes up for the fold is member_start / member_off, n_members + 1 words each; what
// comes down is O(runs + n_ref).  C ABI: svt_bam_index_fold_device, svt_bam_sorted_bgzf_csi_device, svt_bam_index_last_times.

extern "C++" {

namespace svt {
std::vector<uint8_t>& csi_held_bytes();             // (svt_reads.cpp: the calling thread's result for svt_csi_take)
}

// the kernels of the calling thread's last fold here, from HIP events, and the fold's wall time
static thread_local svt_bam_index_times g_bam_index_times;

struct BamIndexCall : TimedCallStream {                      // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_spans;                                      // svt_bam_index_fold_device's upload; the one-call entry's table is the record call's
    RadixSort sort;                                          // the runs' (key, run) pairs (a member, so freed behind drain())
    DevScratch d_member_start, d_member_off, d_s, d_m, d_rkey, d_flag, d_unm, d_tile_heads, d_tile_unmapped, d_tile_top, d_small, d_run_s, d_run_e, d_runs,
        d_loff, d_rows;
    ~BamIndexCall() { drain(); }
};

// d_spans (n rows; d_perm / d_dst_off: svt_bam_index_kernel.h, null for a table in written order): device memory that is filled
// and idle.  -> the bytes of the .csi in `out`, or the 1-based number of the first record the index cannot hold and why
static int fold_resident(BamIndexCall& f, const svt_bam_span* d_spans, const uint64_t* d_perm, const uint64_t* d_dst_off, uint64_t n, int32_t n_ref,
                         uint64_t l_ref_max, const uint64_t* member_start, const uint64_t* member_off, uint64_t n_members, std::vector<uint8_t>& out,
                         uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_bam_index_times = svt_bam_index_times();
    out.clear();
    *bad_record = 0;
    *bad_kind = 0;
    const uint32_t depth = idx::depth_for(l_ref_max);
    const uint64_t end_voff = member_off[n_members] << 16;
    std::vector<idx::Run> runs;
    std::vector<uint64_t> loff;
    std::vector<idx::RefRow> rows((size_t)n_ref, idx::RefRow{0, 0, 0, 0});
    uint64_t no_coor = 0;
    if (n) {
        const uint32_t n_tiles = (uint32_t)((n + kSortTile - 1) / kSortTile);
        const unsigned tile_grid = lines_grid(n_tiles, device);
        SVT_TRY(f.d_member_start.alloc((n_members + 1) * sizeof(uint64_t)));
        SVT_TRY(f.d_member_off.alloc((n_members + 1) * sizeof(uint64_t)));
        SVT_TRY(f.d_s.alloc(n * sizeof(uint64_t)));
        SVT_TRY(f.d_m.alloc(n * sizeof(uint64_t)));
        SVT_TRY(f.d_rkey.alloc(n * sizeof(uint64_t)));
        SVT_TRY(f.d_flag.alloc(n));
        SVT_TRY(f.d_unm.alloc(n * sizeof(uint32_t)));
        SVT_TRY(f.d_tile_heads.alloc(n_tiles * sizeof(uint32_t)));
        SVT_TRY(f.d_tile_unmapped.alloc(n_tiles * sizeof(uint32_t)));
        SVT_TRY(f.d_tile_top.alloc(n_tiles * sizeof(uint64_t)));
        SVT_TRY(f.d_small.alloc(4 * sizeof(uint64_t)));
        SVT_TRY(f.sort.room(n));                                    // the runs' keys and indices: n at the most
        SVT_TRY(f.d_run_s.alloc(n * sizeof(uint64_t)));
        SVT_TRY(f.d_run_e.alloc(n * sizeof(uint64_t)));
        uint64_t small[4] = {~0ull, 0, 0, 0};                       // first refusal (a minimum), records without coordinate, heads, unmapped
        SVT_TRY(h2d_staged(f.d_member_start.p, member_start, (n_members + 1) * sizeof(uint64_t), f.s));
        SVT_TRY(h2d_staged(f.d_member_off.p, member_off, (n_members + 1) * sizeof(uint64_t), f.s));
        SVT_TRY(h2d_staged(f.d_small.p, small, sizeof small, f.s));
        const BamIndexArgs a{d_spans, d_perm, d_dst_off, n, n_ref, depth, f.d_member_start.as<uint64_t>(), f.d_member_off.as<uint64_t>(), n_members};
        size_t e[4] = {};
        SVT_TRY(f.mark(&e[0]));
        hipLaunchKernelGGL(svt_bam_index_record_kernel, dim3(lines_grid((n + kSortBlock - 1) / kSortBlock, device)), dim3(kSortBlock), 0, f.s, a,
                           f.d_s.as<uint64_t>(), f.d_m.as<uint64_t>(), f.d_rkey.as<uint64_t>(), f.d_flag.as<uint8_t>(), f.d_small.as<unsigned long long>(),
                           f.d_small.as<unsigned long long>() + 1);
        HIP_TRY(hipGetLastError());
        SVT_TRY(f.mark(&e[1]));
        hipLaunchKernelGGL(svt_bam_index_partials_kernel, dim3(tile_grid), dim3(kSortBlock), 0, f.s, f.d_m.as<uint64_t>(), f.d_flag.as<uint8_t>(), n, n_tiles,
                           f.d_tile_heads.as<uint32_t>(), f.d_tile_unmapped.as<uint32_t>(), f.d_tile_top.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(svt_bam_index_tiles_kernel, dim3(1), dim3(kSortBlock), 0, f.s, f.d_tile_heads.as<uint32_t>(), f.d_tile_unmapped.as<uint32_t>(),
                           f.d_tile_top.as<uint64_t>(), n_tiles, f.d_small.as<uint64_t>() + 2);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(svt_bam_index_apply_kernel, dim3(tile_grid), dim3(kSortBlock), 0, f.s, f.d_m.as<uint64_t>(), f.d_flag.as<uint8_t>(),
                           f.d_s.as<uint64_t>(), f.d_rkey.as<uint64_t>(), n, n_tiles, f.d_tile_heads.as<uint32_t>(), f.d_tile_unmapped.as<uint32_t>(),
                           f.d_tile_top.as<uint64_t>(), end_voff, f.d_unm.as<uint32_t>(), f.sort.keys(), f.d_run_s.as<uint64_t>(),
                           f.d_run_e.as<uint64_t>(), n);
        HIP_TRY(hipGetLastError());
        SVT_TRY(f.mark(&e[2]));
        SVT_TRY(d2h_staged(small, f.d_small.p, sizeof small, f.s));
        HIP_TRY(hipStreamSynchronize(f.s));
        SVT_TRY(f.between(e[0], e[1], &g_bam_index_times.record_kernel_s));
        SVT_TRY(f.between(e[1], e[2], &g_bam_index_times.scan_kernel_s));
        if (small[0] != ~0ull) {
            *bad_record = small[0] >> 8;
            *bad_kind = (uint32_t)(small[0] & 255);
            if (*bad_record == 0 || *bad_record > n || *bad_kind == 0) return fail(SVT_ERR_HIP, "svt_bam_index_record_kernel: the first refusal names no record");
            g_bam_index_times.total_s = seconds_since(t0);
            return SVT_OK;
        }
        no_coor = small[1];
        const uint64_t n_runs = small[2];
        if (no_coor > n || n_runs > n - no_coor) return fail(SVT_ERR_HIP, "svt_bam_index_tiles_kernel: more runs than placed records");
        const uint64_t n_placed = n - no_coor;
        g_bam_index_times.runs = n_runs;
        if (n_runs) {
            unsigned grid = 0;
            SVT_TRY(f.sort.key_grid(n_runs, device, &grid));
            SVT_TRY(f.d_runs.alloc(n_runs * sizeof(idx::Run)));
            SVT_TRY(f.d_loff.alloc(n_runs * sizeof(uint64_t)));
            SVT_TRY(f.mark(&e[0]));
            hipLaunchKernelGGL(svt_bam_index_run_keys_kernel, dim3(grid), dim3(kSortBlock), 0, f.s, f.sort.keys(), n_runs, f.sort.idx(), f.sort.part_and(),
                               f.sort.part_or());
            HIP_TRY(hipGetLastError());
            SVT_TRY(f.mark(&e[1]));
            SVT_TRY(f.sort.combine(f));
            SVT_TRY(f.between(e[0], e[1], &g_bam_index_times.sort_kernel_s));
            std::vector<uint32_t> order;
            SVT_TRY(f.sort.order(f, order, device));
            double& sort_s = g_bam_index_times.sort_kernel_s;       // the run-key kernel and the three pass kernels summed
            SVT_TRY(f.sort.times(f, &g_bam_index_times.passes, &sort_s, &sort_s, &sort_s));
            SVT_TRY(f.mark(&e[0]));
            hipLaunchKernelGGL(svt_bam_index_loffset_kernel, dim3(grid), dim3(kSortBlock), 0, f.s, f.sort.sorted_keys(), f.sort.sorted_idx(), n_runs,
                               f.d_run_s.as<uint64_t>(), f.d_run_e.as<uint64_t>(), f.d_m.as<uint64_t>(), f.d_s.as<uint64_t>(), n_placed, depth,
                               f.d_runs.as<idx::Run>(), f.d_loff.as<uint64_t>());
            HIP_TRY(hipGetLastError());
            SVT_TRY(f.mark(&e[1]));
            runs.resize(n_runs);
            loff.resize(n_runs);
            SVT_TRY(d2h_staged(runs.data(), f.d_runs.p, n_runs * sizeof(idx::Run), f.s));
            SVT_TRY(d2h_staged(loff.data(), f.d_loff.p, n_runs * sizeof(uint64_t), f.s));
            HIP_TRY(hipStreamSynchronize(f.s));
            SVT_TRY(f.between(e[0], e[1], &g_bam_index_times.loffset_kernel_s));
        }
        if (n_ref) {
            SVT_TRY(f.d_rows.alloc((uint64_t)n_ref * sizeof(idx::RefRow)));
            SVT_TRY(f.mark(&e[0]));
            hipLaunchKernelGGL(svt_bam_index_reference_kernel, dim3(lines_grid(((uint64_t)n_ref + kSortBlock - 1) / kSortBlock, device)), dim3(kSortBlock), 0, f.s,
                               f.d_m.as<uint64_t>(), f.d_s.as<uint64_t>(), f.d_unm.as<uint32_t>(), n, n_placed, (uint64_t)n_ref, end_voff,
                               f.d_rows.as<idx::RefRow>());
            HIP_TRY(hipGetLastError());
            SVT_TRY(f.mark(&e[1]));
            SVT_TRY(d2h_staged(rows.data(), f.d_rows.p, (uint64_t)n_ref * sizeof(idx::RefRow), f.s));
            HIP_TRY(hipStreamSynchronize(f.s));
            SVT_TRY(f.between(e[0], e[1], &g_bam_index_times.reference_kernel_s));
        }
        // what came down is sorted runs with their group heads' loffsets and the references' rows, or it is not the kernels':
        // what the serialiser relies on
        uint64_t in_runs = 0;
        for (uint64_t q = 0; q < n_runs; ++q) {
            const idx::Run& r = runs[q];
            const bool head = q == 0 || runs[q - 1].key != r.key;
            if (q && (runs[q - 1].key > r.key || (!head && runs[q - 1].e > r.s))) return fail(SVT_ERR_HIP, "svt_bam_index_loffset_kernel: the runs are not sorted");
            if (r.s > r.e || r.e > end_voff || r.key >> 32 >= (uint64_t)n_ref) return fail(SVT_ERR_HIP, "svt_bam_index_loffset_kernel: a run is none of the stream's");
            if (head && loff[q] > r.s) return fail(SVT_ERR_HIP, "svt_bam_index_loffset_kernel: a loffset lies behind its bin's first record");
            const idx::RefRow& row = rows[(size_t)(r.key >> 32)];
            if (row.mapped + row.unmapped == 0 || r.s < row.first || r.e > row.last) return fail(SVT_ERR_HIP, "svt_bam_index_reference_kernel: a run outside its reference's records");
        }
        for (const idx::RefRow& row : rows) {
            if (row.first > row.last || row.last > end_voff) return fail(SVT_ERR_HIP, "svt_bam_index_reference_kernel: a reference's records are none of the stream's");
            in_runs += row.mapped + row.unmapped;
        }
        if (in_runs != n_placed) return fail(SVT_ERR_HIP, "svt_bam_index_reference_kernel: the references' records are not the placed records");
    }
    tbx::Builder b;
    csi::serialise(b, depth, std::vector<uint8_t>(), (uint64_t)n_ref, runs.data(), runs.size(), loff.data(), rows.data(), no_coor);
    out.swap(b.out);
    g_bam_index_times.total_s = seconds_since(t0);
    return SVT_OK;
}

// what the fold asks of its tables (bai::check_tables, svt_csi_build_bam's), in the entry's name
static int fold_check_tables(const char* entry, const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                             const uint64_t* member_off, uint64_t n_members)
{
    if (n >> 32) return fail(SVT_ERR_INVALID, std::string(entry) + ": too many records in one call (< 2^32)");
    if (const char* why = bai::check_tables(spans, n, n_ref, l_ref_max, member_start, member_off, n_members))
        return fail(SVT_ERR_INVALID, std::string(entry) + ": " + why);
    return SVT_OK;
}

static int svt_bam_index_fold_device_impl(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                                          const uint64_t* member_off, uint64_t n_members, uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    if ((n && !spans) || !member_start || !member_off || !size || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
    SVT_TRY(fold_check_tables("svt_bam_index_fold", spans, n, n_ref, l_ref_max, member_start, member_off, n_members));
    *size = 0;
    std::vector<uint8_t>& held = csi_held_bytes();
    held.clear();
    SVT_TRY(select_device(device));
    BamIndexCall f;
    SVT_TRY(f.take());
    if (n) {
        SVT_TRY(f.d_spans.alloc(n * sizeof(svt_bam_span)));
        SVT_TRY(h2d_staged(f.d_spans.p, spans, n * sizeof(svt_bam_span), f.s));
    }
    SVT_TRY(fold_resident(f, f.d_spans.as<svt_bam_span>(), nullptr, nullptr, n, n_ref, l_ref_max, member_start, member_off, n_members, held, bad_record, bad_kind,
                          device));
    *size = held.size();
    return SVT_OK;
}

static int svt_bam_sorted_bgzf_csi_device_impl(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, uint64_t l_ref_max,
                                               int sort, uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint64_t member_capacity,
                                               uint64_t* n_members, uint64_t* member_start, svt_bam_span* spans, uint64_t* perm, uint64_t* bad_record,
                                               uint32_t* bad_kind, uint64_t* csi_size, uint64_t* index_bad_record, uint32_t* index_bad_kind, int device)
{
    if (!csi_size || !index_bad_record || !index_bad_kind) return fail(SVT_ERR_INVALID, "null argument");
    if (l_ref_max >> 32) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf_csi: l_ref_max is below 2^32");
    *csi_size = 0;
    *index_bad_record = 0;
    *index_bad_kind = 0;
    std::vector<uint8_t>& held = csi_held_bytes();
    held.clear();
    // behind the members, while the span table, the order and the records' places in the written stream are resident: the fold
    const BamFoldHook hook = [&](BamSortCall& c, bool sorted, uint64_t members) -> int {
        HIP_TRY(hipStreamSynchronize(c.s));
        SVT_TRY(fold_check_tables("svt_bam_sorted_bgzf_csi", nullptr, n, n_ref, l_ref_max, member_start, out_off, members));
        BamIndexCall f;
        SVT_TRY(f.take());
        SVT_TRY(fold_resident(f, c.d_spans.as<svt_bam_span>(), sorted ? c.d_perm.as<uint64_t>() : nullptr, sorted ? c.d_dst_off.as<uint64_t>() : nullptr, n, n_ref,
                              l_ref_max, member_start, out_off, members, held, index_bad_record, index_bad_kind, device));
        *csi_size = held.size();
        return SVT_OK;
    };
    return svt_bam_sorted_bgzf_device_impl(bytes, len, rec_off, n, n_ref, sort, mode, out, capacity, out_off, member_capacity, n_members, member_start, spans,
                                           perm, bad_record, bad_kind, device, &hook);
}

}  // extern "C++"

int svt_bam_index_fold_device(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                              const uint64_t* member_off, uint64_t n_members, uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    return guarded([&] { return svt_bam_index_fold_device_impl(spans, n, n_ref, l_ref_max, member_start, member_off, n_members, size, bad_record, bad_kind, device); });
}

int svt_bam_sorted_bgzf_csi_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, uint64_t l_ref_max, int sort,
                                   uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint64_t member_capacity, uint64_t* n_members,
                                   uint64_t* member_start, svt_bam_span* spans, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, uint64_t* csi_size,
                                   uint64_t* index_bad_record, uint32_t* index_bad_kind, int device)
{
    return guarded([&] {
        return svt_bam_sorted_bgzf_csi_device_impl(bytes, len, rec_off, n, n_ref, l_ref_max, sort, mode, out, capacity, out_off, member_capacity, n_members,
                                                   member_start, spans, perm, bad_record, bad_kind, csi_size, index_bad_record, index_bad_kind, device);
    });
}

int svt_bam_index_last_times(svt_bam_index_times* times) { return guarded([&] { return last_times(times, g_bam_index_times); }); }

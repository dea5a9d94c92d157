// svt_entry_vcf_group.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_radix_sort.h; not a stand-alone header): BND mates grouped on the device.  One call: the text and the FORMAT table go
// up once and the line table is made (cohort_begin, svt_entry_vcf_cohort.h), svt_group_scan_kernel writes the records, the BND
// lines are compacted by a scan and their (ID hash, line) pairs go through the call's RadixSort (svt_entry_radix_sort.h: the one sort, not a copy of it),
// svt_group_match_kernel joins, and for a regular file without marked lines a second scan and svt_group_plan_kernel write the
// plan: the records and the plan come down.  Any marked line, or a file that is not regular: only the records come down and
// group::join, the host twin's, finishes (report->host_join).  C ABI: svt_vcf_group_device, svt_vcf_group_last_times
// (include/svtyper_reads.h); the host twin and the writer are in svt_reads_group_entries.h.

extern "C++" {

static thread_local svt_vcf_group_times g_group_times;

struct GroupCall : CohortCall {                              // (d_tables: the FORMAT table, d_results: the records; destruction order: CallStream)
    DevScratch d_bnd, d_emit, d_mate, d_status, d_plan;
    RadixSort sort;                                          // (a member, so freed behind drain())
    ~GroupCall() { drain(); }
};

static int svt_vcf_group_device_impl(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                                     svt_group_line* lines, uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan,
                                     svt_group_report* report, uint32_t hash_bits, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    svt_vcf_group_times& times = g_group_times;
    times = svt_vcf_group_times();
    g_lines_times = svt_vcf_lines_times();
    group::Block b;
    if (const char* why = group::take_arguments(text, len, n_samples, format_table, format_len, lines, n_lines, plan, n_plan, report, b))
        return fail(SVT_ERR_INVALID, why);
    if (hash_bits < 1 || hash_bits > 64) return fail(SVT_ERR_INVALID, "svt_vcf_group: hash_bits is 1..64");
    *n_plan = 0;
    GroupCall c;
    std::vector<svt_tbx_line> table;
    SVT_TRY(cohort_begin(c, b, format_table, format_len, table, capacity, n_lines, device, times));
    if (table.empty()) return SVT_OK;
    const uint64_t n = table.size(), mask = bfr::hash_mask(hash_bits);
    if (n >> 31) return fail(SVT_ERR_INVALID, "svt_vcf_group: too many lines in one call (< 2^31)");
    SVT_TRY(c.d_results.alloc(n * sizeof(svt_group_line)));
    SVT_TRY(c.d_bnd.alloc((n + 1) * sizeof(uint32_t)));
    SVT_TRY(c.d_emit.alloc((n + 1) * sizeof(uint32_t)));
    SVT_TRY(c.d_mate.alloc(n * sizeof(uint32_t)));
    SVT_TRY(c.d_status.alloc(sizeof(GroupStatus)));
    HIP_TRY(hipMemsetAsync(c.d_bnd.p, 0, (n + 1) * sizeof(uint32_t), c.s));
    HIP_TRY(hipMemsetAsync(c.d_emit.p, 0, (n + 1) * sizeof(uint32_t), c.s));
    HIP_TRY(hipMemsetAsync(c.d_mate.p, 0xFF, n * sizeof(uint32_t), c.s));
    GroupStatus status = {kGroupNoFatal, 0, 0};
    SVT_TRY(h2d_staged(c.d_status.p, &status, sizeof status, c.s));
    const unsigned grid = lines_grid((n + kSortBlock - 1) / kSortBlock, device);
    size_t e[9] = {};
    SVT_TRY(c.mark(&e[0]));
    hipLaunchKernelGGL(svt_group_scan_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n,
                       c.d_tables.as<uint8_t>(), (uint32_t)format_len, c.d_results.as<svt_group_line>(), c.d_bnd.as<uint32_t>(), c.d_emit.as<uint32_t>(),
                       c.d_status.as<GroupStatus>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    hipLaunchKernelGGL(svt_bam_scan_kernel, dim3(1), dim3(kSortBlock), 0, c.s, c.d_bnd.as<uint32_t>(), n + 1);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[2]));
    uint32_t n_bnd = 0;
    SVT_TRY(d2h_staged(&status, c.d_status.p, sizeof status, c.s));
    SVT_TRY(d2h_staged(&n_bnd, c.d_bnd.as<uint32_t>() + n, sizeof n_bnd, c.s));
    SVT_TRY(c.between(e[0], e[1], &times.scan_kernel_s));
    SVT_TRY(c.between(e[1], e[2], &times.compact_kernels_s));
    if (n_bnd > n) return fail(SVT_ERR_HIP, "svt_group_scan_kernel: more BND lines than lines");
    bool on_device = !status.any_slow;
    if (on_device && n_bnd) {
        unsigned key_grid = 0;
        SVT_TRY(c.sort.room(n_bnd));
        SVT_TRY(c.sort.key_grid(n_bnd, n, device, &key_grid));      // (n_bnd pairs from a key kernel that walks the n lines)
        SVT_TRY(c.mark(&e[3]));
        hipLaunchKernelGGL(svt_group_compact_kernel, dim3(key_grid), dim3(kSortBlock), 0, c.s, c.d_stream.as<uint8_t>(), len,
                           c.d_results.as<svt_group_line>(), n, c.d_bnd.as<uint32_t>(), (uint64_t)n_bnd, mask, c.sort.keys(), c.sort.idx(),
                           c.sort.part_and(), c.sort.part_or());
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[4]));
        SVT_TRY(c.sort.combine(c));
        SVT_TRY(c.between(e[3], e[4], &times.compact_kernels_s));
        SVT_TRY(c.sort.passes(c, device));
        SVT_TRY(c.mark(&e[5]));
        hipLaunchKernelGGL(svt_group_match_kernel, dim3(lines_grid((n_bnd + kSortBlock - 1) / kSortBlock, device)), dim3(kSortBlock), 0, c.s,
                           c.d_stream.as<uint8_t>(), len, c.d_results.as<svt_group_line>(), n, c.sort.sorted_keys(), c.sort.sorted_idx(), (uint64_t)n_bnd,
                           mask, c.d_emit.as<uint32_t>(), c.d_mate.as<uint32_t>(), c.d_status.as<GroupStatus>());
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[6]));
        SVT_TRY(d2h_staged(&status, c.d_status.p, sizeof status, c.s));
        uint32_t passes = 0;
        SVT_TRY(c.sort.times(c, &passes, &times.sort_kernels_s, &times.sort_kernels_s, &times.sort_kernels_s));
        SVT_TRY(c.between(e[5], e[6], &times.match_kernel_s));
        on_device = !status.irregular;
    }
    if (!on_device) {                               // the records alone: the host twin's join finishes
        auto t = std::chrono::steady_clock::now();
        SVT_TRY(d2h_staged(lines, c.d_results.p, n * sizeof(svt_group_line), c.s));
        times.download_s = seconds_since(t);
        t = std::chrono::steady_clock::now();
        if (!group::records_inside(b, lines, n)) return fail(SVT_ERR_HIP, "svt_group_scan_kernel: a record's line is not inside the text");
        group::join(b, lines, n, plan, n_plan, *report);
        times.host_s = seconds_since(t);
        times.total_s = seconds_since(t0);
        return SVT_OK;
    }
    const uint64_t fatal = std::min<uint64_t>(status.fatal, n);
    SVT_TRY(c.d_plan.alloc(2 * n * sizeof(svt_group_out)));
    HIP_TRY(hipMemsetAsync(c.d_plan.p, 0xFF, 2 * n * sizeof(svt_group_out), c.s));
    SVT_TRY(c.mark(&e[7]));
    hipLaunchKernelGGL(svt_bam_scan_kernel, dim3(1), dim3(kSortBlock), 0, c.s, c.d_emit.as<uint32_t>(), n + 1);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(svt_group_plan_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, c.d_emit.as<uint32_t>(), c.d_mate.as<uint32_t>(), n, fatal,
                       c.d_plan.as<svt_group_out>(), 2 * n);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[8]));
    uint32_t total = 0;
    SVT_TRY(d2h_staged(&total, c.d_emit.as<uint32_t>() + fatal, sizeof total, c.s));
    SVT_TRY(c.between(e[7], e[8], &times.plan_kernels_s));
    if (total > 2 * n) return fail(SVT_ERR_HIP, "svt_group_plan_kernel: more entries than twice the lines");
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(lines, c.d_results.p, n * sizeof(svt_group_line), c.s));
    if (total) SVT_TRY(d2h_staged(plan, c.d_plan.p, total * sizeof(svt_group_out), c.s));
    times.download_s = seconds_since(t);
    t = std::chrono::steady_clock::now();
    // every entry was written and names lines in front of the fatal one, or the plan is not the kernels'
    for (uint32_t j = 0; j < total; ++j)
        if (plan[j].line >= fatal || plan[j].source > plan[j].line) return fail(SVT_ERR_HIP, "svt_group_plan_kernel: an entry was not written");
    *n_plan = total;
    report->n_bnd = n_bnd;
    if (fatal < n) {                                // inside the envelope a line ends the run for a missing key alone
        const svt_group_line& l = lines[fatal];
        cohort::report(*report, fatal + 1, l.bad ? group::bad_key(l.bad & 255u, l.bad >> 8) : group::bad_key(SVT_GROUP_BAD_KEY, SVT_GROUP_KEY_CIPOS));
    }
    times.host_s = seconds_since(t);
    times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_vcf_group_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len, svt_group_line* lines,
                         uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan, svt_group_report* report, uint32_t hash_bits,
                         int device)
{
    return guarded([&] {
        return svt_vcf_group_device_impl(text, len, n_samples, format_table, format_len, lines, capacity, n_lines, plan, n_plan, report, hash_bits, device);
    });
}

int svt_vcf_group_last_times(svt_vcf_group_times* times) { return guarded([&] { return last_times(times, g_group_times); }); }

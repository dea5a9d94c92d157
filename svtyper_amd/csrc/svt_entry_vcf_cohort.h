// svt_entry_vcf_cohort.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_lines.h; not a stand-alone header): one device call of a rule over the lines of a cohort VCF, for
// svt_entry_vcf_classify.h and svt_entry_vcf_update_info.h.  The text and the rule's tables go up, the line table is made
// (lines_resident), the rule's kernel runs, the records come down and the marked lines are settled on the host (cohort::settle).

extern "C++" {

struct CohortCall : LinesCall {                              // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_tables, d_results;
    ~CohortCall() { drain(); }
};

// `b` holds the checked arguments; `times` is the rule's svt_vcf_*_times, `kernel_s` its field for the rule's kernel;
// launch(c, grid, n) starts that kernel over the n lines of c.d_lines with the tables in c.d_tables
template <class Block, class Line, class Info, class Times, class Launch>
static int cohort_device(Block& b, const uint8_t* tables, size_t tables_len, Line* results, uint64_t capacity, uint64_t* n_lines, Info& info, int device,
                         std::chrono::steady_clock::time_point t0, Times& times, double& kernel_s, Launch launch)
{
    *n_lines = 0;
    SVT_TRY(select_device(device));
    if (!b.len) return SVT_OK;
    CohortCall c;
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(c.begin(b.text, b.len));
    SVT_TRY(c.d_tables.alloc(tables_len));
    SVT_TRY(h2d_staged(c.d_tables.p, tables, tables_len, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    times.upload_s = seconds_since(t);
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, b.len, b.text[b.len - 1], table, device));
    times.lines_kernels_s = g_lines_times.count_kernel_s + g_lines_times.starts_kernel_s + g_lines_times.parse_kernel_s;
    *n_lines = table.size();
    if (table.size() > capacity) return fail(SVT_ERR_INVALID, Block::kCapacityWhy);
    b.lines = table.data();
    b.n_table = table.size();
    const uint64_t n = table.size();
    SVT_TRY(c.d_results.alloc(n * sizeof(Line)));
    const unsigned grid = (unsigned)std::max<uint64_t>(std::min<uint64_t>(n, (uint64_t)std::max<uint32_t>(cu_count(device), 1) * 12), 1);
    size_t e[2] = {};
    SVT_TRY(c.mark(&e[0]));
    launch(c, grid, n);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    HIP_TRY(hipStreamSynchronize(c.s));             // (the download's clock starts behind the kernel, not with it)
    t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(results, c.d_results.p, n * sizeof(Line), c.s));
    times.download_s = seconds_since(t);
    SVT_TRY(c.between(e[0], e[1], &kernel_s));
    t = std::chrono::steady_clock::now();
    cohort::settle(b, results, info);
    times.host_s = seconds_since(t);
    times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

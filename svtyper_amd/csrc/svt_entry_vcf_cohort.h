// svt_entry_vcf_cohort.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_lines.h; not a stand-alone header): one device call over the lines of a cohort VCF.  cohort_begin is the part of it
// that every such call starts with: the text and the call's tables go up and the line table is made (lines_resident).
// cohort_device is the whole call of a rule over single lines, for svt_entry_vcf_classify.h and svt_entry_vcf_update_info.h:
// cohort_begin, the rule's kernel, the records down and the marked lines settled on the host (cohort::settle).
// svt_entry_vcf_group.h puts its join behind cohort_begin.

extern "C++" {

struct CohortCall : LinesCall {                              // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_tables, d_results;
    ~CohortCall() { drain(); }
};

// `b` holds the checked arguments, `times` is the rule's svt_vcf_*_times.  Behind it the text is in c.d_stream, the tables are in
// c.d_tables, the line table is in c.d_lines and in `table`, with b.lines and *n_lines naming it.  An empty text starts nothing and
// leaves `table` empty: the call is over
template <class Block, class Times>
static int cohort_begin(CohortCall& c, Block& b, const uint8_t* tables, size_t tables_len, std::vector<svt_tbx_line>& table, uint64_t capacity,
                        uint64_t* n_lines, int device, Times& times)
{
    *n_lines = 0;
    SVT_TRY(select_device(device));
    if (!b.len) return SVT_OK;
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(c.begin(b.text, b.len));
    SVT_TRY(c.d_tables.alloc(tables_len));
    SVT_TRY(h2d_staged(c.d_tables.p, tables, tables_len, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    times.upload_s = seconds_since(t);
    SVT_TRY(lines_resident(c, b.len, b.text[b.len - 1], table, device));
    times.lines_kernels_s = lines_kernels_s();
    *n_lines = table.size();
    if (table.size() > capacity) return fail(SVT_ERR_INVALID, Block::kCapacityWhy);
    b.lines = table.data();
    b.n_table = table.size();
    return SVT_OK;
}

// `kernel_s` is the field of `times` for the rule's kernel; launch(c, grid, n) starts that kernel over the n lines of c.d_lines
// with the tables in c.d_tables
template <class Block, class Line, class Info, class Times, class Launch>
static int cohort_device(Block& b, const uint8_t* tables, size_t tables_len, Line* results, uint64_t capacity, uint64_t* n_lines, Info& info, int device,
                         std::chrono::steady_clock::time_point t0, Times& times, double& kernel_s, Launch launch)
{
    CohortCall c;
    std::vector<svt_tbx_line> table;
    SVT_TRY(cohort_begin(c, b, tables, tables_len, table, capacity, n_lines, device, times));
    if (table.empty()) return SVT_OK;
    const uint64_t n = table.size();
    SVT_TRY(c.d_results.alloc(n * sizeof(Line)));
    const unsigned grid = capped_grid(n, 12, device);
    size_t e[2] = {};
    SVT_TRY(c.mark(&e[0]));
    launch(c, grid, n);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    HIP_TRY(hipStreamSynchronize(c.s));             // (the download's clock starts behind the kernel, not with it)
    auto t = std::chrono::steady_clock::now();
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

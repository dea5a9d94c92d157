// svt_entry_vcf_classify.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_paste.h; not a stand-alone header): the read-depth classifier of DEL and DUP lines on the device.  What is this
// header's: the launch of svt_vcf_classify_kernel.h, the per-sample tables' upload, the marked lines settled on the host
// (classify::settle_block), the times.  What it shares lives in svt_entry_vcf_lines.h (the line table: lines_resident) and
// svt_entry_deflate.h (the upload: OrderedCall::begin).  Only the records come down: the output text is written on the host, which
// holds the input (svt_vcf_classify_write).  C ABI: svt_vcf_classify_device, svt_vcf_classify_last_times (include/svtyper_reads.h).

extern "C++" {

static thread_local svt_vcf_classify_times g_classify_times;

struct ClassifyCall : LinesCall {                            // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_tables, d_results;
    ~ClassifyCall() { drain(); }
};

static int svt_vcf_classify_device_impl(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                                        const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip,
                                        double slope_threshold, double rsquared_threshold, svt_classify_line* results, uint64_t capacity,
                                        uint64_t* n_lines, svt_classify_info* info, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_classify_times = svt_vcf_classify_times();
    g_lines_times = svt_vcf_lines_times();
    classify::Block b;
    if (const char* why = classify::take_arguments(text, len, n_samples, male, female, excluded, format_table, format_len, skip, slope_threshold,
                                                   rsquared_threshold, results, n_lines, info, b))
        return fail(SVT_ERR_INVALID, why);
    *n_lines = 0;
    SVT_TRY(select_device(device));
    if (!len) return SVT_OK;
    ClassifyCall c;
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(c.begin(text, len));
    // male, female, excluded [n_samples] and the FORMAT ids side by side
    std::vector<uint8_t> tables(3 * (size_t)n_samples + format_len);
    if (n_samples) {
        std::memcpy(tables.data(), male, n_samples);
        std::memcpy(tables.data() + n_samples, female, n_samples);
        std::memcpy(tables.data() + 2 * (size_t)n_samples, excluded, n_samples);
    }
    std::memcpy(tables.data() + 3 * (size_t)n_samples, format_table, format_len);
    SVT_TRY(c.d_tables.alloc(tables.size()));
    SVT_TRY(h2d_staged(c.d_tables.p, tables.data(), tables.size(), c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    g_classify_times.upload_s = seconds_since(t);
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, text[len - 1], table, device));
    g_classify_times.lines_kernels_s = g_lines_times.count_kernel_s + g_lines_times.starts_kernel_s + g_lines_times.parse_kernel_s;
    *n_lines = table.size();
    if (table.size() > capacity) return fail(SVT_ERR_INVALID, "svt_vcf_classify: capacity is below the number of lines");
    b.lines = table.data();
    b.n_table = table.size();
    const uint64_t n = table.size();
    SVT_TRY(c.d_results.alloc(n * sizeof(svt_classify_line)));
    const unsigned grid = (unsigned)std::max<uint64_t>(std::min<uint64_t>(n, (uint64_t)std::max<uint32_t>(cu_count(device), 1) * 12), 1);
    size_t e[2] = {};
    SVT_TRY(c.mark(&e[0]));
    const uint8_t* d = c.d_tables.as<uint8_t>();
    hipLaunchKernelGGL(svt_classify_kernel, dim3(grid), dim3(kClassifyBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n, d,
                       d + n_samples, d + 2 * (size_t)n_samples, d + 3 * (size_t)n_samples, b.pr, c.d_results.as<svt_classify_line>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    HIP_TRY(hipStreamSynchronize(c.s));             // (the download's clock starts behind the kernel, not with it)
    t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(results, c.d_results.p, n * sizeof(svt_classify_line), c.s));
    g_classify_times.download_s = seconds_since(t);
    SVT_TRY(c.between(e[0], e[1], &g_classify_times.classify_kernel_s));
    t = std::chrono::steady_clock::now();
    classify::Bad bad;
    if (const uint64_t bad_line = classify::settle_block(b, results, *info, bad)) classify::report(*info, bad_line, bad);
    g_classify_times.host_s = seconds_since(t);
    g_classify_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_vcf_classify_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                            const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip, double slope_threshold,
                            double rsquared_threshold, svt_classify_line* results, uint64_t capacity, uint64_t* n_lines, svt_classify_info* info,
                            int device)
{
    return guarded([&] {
        return svt_vcf_classify_device_impl(text, len, n_samples, male, female, excluded, format_table, format_len, skip, slope_threshold,
                                            rsquared_threshold, results, capacity, n_lines, info, device);
    });
}

int svt_vcf_classify_last_times(svt_vcf_classify_times* times) { return guarded([&] { return last_times(times, g_classify_times); }); }

// svt_entry_vcf_update_info.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_classify.h; not a stand-alone header): PE, SR, SU and MSQ of a cohort VCF's lines on the device.  What is this
// header's: the launch of svt_vcf_update_info_kernel.h (the kernel and update_info_launch are svt_small_kernels.hip's), the FORMAT
// table's upload, the marked lines settled on the host (update_info::settle_block), the times.  What it shares lives in
// svt_entry_vcf_lines.h (the line table: lines_resident) and svt_entry_deflate.h (the upload: OrderedCall::begin).  Only the
// records come down: the output text is written on the host, which holds the input (svt_vcf_update_info_write).  C ABI:
// svt_vcf_update_info_device, svt_vcf_update_info_last_times (include/svtyper_reads.h).

extern "C++" {

namespace svt {
void update_info_launch(unsigned grid, hipStream_t stream, const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n_lines,
                        const uint8_t* format_table, uint32_t n_samples, uint32_t format_len, svt_update_info_line* results);
}

static thread_local svt_vcf_update_info_times g_update_info_times;

struct UpdateInfoCall : LinesCall {                          // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_table, d_results;
    ~UpdateInfoCall() { drain(); }
};

static int svt_vcf_update_info_device_impl(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                                           svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines, svt_update_info_report* info,
                                           int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_update_info_times = svt_vcf_update_info_times();
    g_lines_times = svt_vcf_lines_times();
    update_info::Block b;
    if (const char* why = update_info::take_arguments(text, len, n_samples, format_table, format_len, results, n_lines, info, b))
        return fail(SVT_ERR_INVALID, why);
    *n_lines = 0;
    SVT_TRY(select_device(device));
    if (!len) return SVT_OK;
    UpdateInfoCall c;
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(c.begin(text, len));
    SVT_TRY(c.d_table.alloc(format_len));
    SVT_TRY(h2d_staged(c.d_table.p, format_table, format_len, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    g_update_info_times.upload_s = seconds_since(t);
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, text[len - 1], table, device));
    g_update_info_times.lines_kernels_s = g_lines_times.count_kernel_s + g_lines_times.starts_kernel_s + g_lines_times.parse_kernel_s;
    *n_lines = table.size();
    if (table.size() > capacity) return fail(SVT_ERR_INVALID, "svt_vcf_update_info: capacity is below the number of lines");
    b.lines = table.data();
    b.n_table = table.size();
    const uint64_t n = table.size();
    SVT_TRY(c.d_results.alloc(n * sizeof(svt_update_info_line)));
    const unsigned grid = (unsigned)std::max<uint64_t>(std::min<uint64_t>(n, (uint64_t)std::max<uint32_t>(cu_count(device), 1) * 12), 1);
    size_t e[2] = {};
    SVT_TRY(c.mark(&e[0]));
    update_info_launch(grid, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n, c.d_table.as<uint8_t>(), n_samples,
                       (uint32_t)format_len, c.d_results.as<svt_update_info_line>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    HIP_TRY(hipStreamSynchronize(c.s));             // (the download's clock starts behind the kernel, not with it)
    t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(results, c.d_results.p, n * sizeof(svt_update_info_line), c.s));
    g_update_info_times.download_s = seconds_since(t);
    SVT_TRY(c.between(e[0], e[1], &g_update_info_times.update_info_kernel_s));
    t = std::chrono::steady_clock::now();
    update_info::Bad bad;
    if (const uint64_t bad_line = update_info::settle_block(b, results, *info, bad)) update_info::report(*info, bad_line, bad);
    g_update_info_times.host_s = seconds_since(t);
    g_update_info_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_vcf_update_info_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                               svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines, svt_update_info_report* info, int device)
{
    return guarded([&] {
        return svt_vcf_update_info_device_impl(text, len, n_samples, format_table, format_len, results, capacity, n_lines, info, device);
    });
}

int svt_vcf_update_info_last_times(svt_vcf_update_info_times* times) { return guarded([&] { return last_times(times, g_update_info_times); }); }

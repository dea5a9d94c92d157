// svt_entry_vcf_classify.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_cohort.h; not a stand-alone header): the read-depth classifier of DEL and DUP lines on the device.  What is this
// header's: the per-sample tables that go up, the launch of svt_vcf_classify_kernel.h, the times.  The call itself is
// cohort_device (svt_entry_vcf_cohort.h).  Only the records come down: the output text is written on the host, which holds the
// input (svt_vcf_classify_write).  C ABI: svt_vcf_classify_device, svt_vcf_classify_last_times (include/svtyper_reads.h).

extern "C++" {
static thread_local svt_vcf_classify_times g_classify_times;
}

int svt_vcf_classify_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                            const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip, double slope_threshold,
                            double rsquared_threshold, svt_classify_line* results, uint64_t capacity, uint64_t* n_lines, svt_classify_info* info,
                            int device)
{
    return guarded([&]() -> int {
        const auto t0 = std::chrono::steady_clock::now();
        g_classify_times = svt_vcf_classify_times();
        g_lines_times = svt_vcf_lines_times();
        classify::Block b;
        if (const char* why = classify::take_arguments(text, len, n_samples, male, female, excluded, format_table, format_len, skip, slope_threshold,
                                                       rsquared_threshold, results, n_lines, info, b))
            return fail(SVT_ERR_INVALID, why);
        // male, female, excluded [n_samples] and the FORMAT ids side by side
        std::vector<uint8_t> tables(3 * (size_t)n_samples + format_len);
        if (n_samples) {
            std::memcpy(tables.data(), male, n_samples);
            std::memcpy(tables.data() + n_samples, female, n_samples);
            std::memcpy(tables.data() + 2 * (size_t)n_samples, excluded, n_samples);
        }
        std::memcpy(tables.data() + 3 * (size_t)n_samples, format_table, format_len);
        return cohort_device(b, tables.data(), tables.size(), results, capacity, n_lines, *info, device, t0, g_classify_times,
                             g_classify_times.classify_kernel_s, [&](CohortCall& c, unsigned grid, uint64_t n) {
                                 const uint8_t* d = c.d_tables.as<uint8_t>();
                                 hipLaunchKernelGGL(svt_classify_kernel, dim3(grid), dim3(kClassifyBlock), 0, c.s, c.d_stream.as<uint8_t>(), len,
                                                    c.d_lines.as<svt_tbx_line>(), n, d, d + n_samples, d + 2 * (size_t)n_samples,
                                                    d + 3 * (size_t)n_samples, b.pr, c.d_results.as<svt_classify_line>());
                             });
    });
}

int svt_vcf_classify_last_times(svt_vcf_classify_times* times) { return guarded([&] { return last_times(times, g_classify_times); }); }

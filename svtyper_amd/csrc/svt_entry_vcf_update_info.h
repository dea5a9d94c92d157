// svt_entry_vcf_update_info.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_classify.h; not a stand-alone header): PE, SR, SU and MSQ of a cohort VCF's lines on the device.  What is this
// header's: the FORMAT table that goes up, the launch of svt_vcf_update_info_kernel.h (the kernel and update_info_launch are
// svt_small_kernels.hip's), the times.  The call itself is cohort_device (svt_entry_vcf_cohort.h).  Only the records come down:
// the output text is written on the host, which holds the input (svt_vcf_update_info_write).  C ABI:
// svt_vcf_update_info_device, svt_vcf_update_info_last_times (include/svtyper_reads.h).

extern "C++" {
namespace svt {
void update_info_launch(unsigned grid, hipStream_t stream, const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n_lines,
                        const uint8_t* format_table, uint32_t n_samples, uint32_t format_len, svt_update_info_line* results);
}
static thread_local svt_vcf_update_info_times g_update_info_times;
}

int svt_vcf_update_info_device(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                               svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines, svt_update_info_report* info, int device)
{
    return guarded([&]() -> int {
        const auto t0 = std::chrono::steady_clock::now();
        g_update_info_times = svt_vcf_update_info_times();
        g_lines_times = svt_vcf_lines_times();
        update_info::Block b;
        if (const char* why = update_info::take_arguments(text, len, n_samples, format_table, format_len, results, n_lines, info, b))
            return fail(SVT_ERR_INVALID, why);
        return cohort_device(b, format_table, format_len, results, capacity, n_lines, *info, device, t0, g_update_info_times,
                             g_update_info_times.update_info_kernel_s, [&](CohortCall& c, unsigned grid, uint64_t n) {
                                 update_info_launch(grid, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n,
                                                    c.d_tables.as<uint8_t>(), n_samples, (uint32_t)format_len,
                                                    c.d_results.as<svt_update_info_line>());
                             });
    });
}

int svt_vcf_update_info_last_times(svt_vcf_update_info_times* times) { return guarded([&] { return last_times(times, g_update_info_times); }); }

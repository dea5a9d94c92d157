// svt_reads_update_info_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone
// header): the host entry points of svt_vcf_update_info.h: the records on the host, and the writer of the output text that both
// engines' records go through (svt_reads_cohort_entries.h); the device's entry is in svt_entry_vcf_update_info.h.
extern "C" {

int svt_vcf_update_info_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                             svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines, svt_update_info_report* info)
{
    return guarded([&]() -> int {
        svt::update_info::Block b;
        if (const char* why = svt::update_info::take_arguments(text, len, n_samples, format_table, format_len, results, n_lines, info, b))
            return fail(SVT_ERR_INVALID, why);
        std::vector<svt_tbx_line> table;
        if (const char* why = svt::update_info::update_info_host(b, table, results, capacity, n_lines, *info)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

int svt_vcf_update_info_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                              const uint8_t* format_table, uint64_t format_len, const svt_update_info_line* results, uint64_t n_lines,
                              uint64_t* out_off, svt_update_info_report* info)
{
    return cohort_write<svt::update_info::Block>(text, len, n_samples, info_table, info_len, format_table, format_len, results, n_lines, out_off, info);
}

int svt_vcf_update_info_take(uint8_t* out, uint64_t capacity) { return cohort_take<svt::update_info::Block, svt_update_info_line>(out, capacity); }

}  // extern "C"

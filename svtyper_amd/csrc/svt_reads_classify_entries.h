// svt_reads_classify_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header):
// the host entry points of the read-depth classifier (svt_vcf_classify.h): the records on the host, and the writer of the output
// text that both engines' records go through (svt_reads_cohort_entries.h); the device's entry is in svt_entry_vcf_classify.h.
extern "C" {

int svt_vcf_classify_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                          const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip, double slope_threshold,
                          double rsquared_threshold, svt_classify_line* results, uint64_t capacity, uint64_t* n_lines, svt_classify_info* info)
{
    return guarded([&]() -> int {
        svt::classify::Block b;
        if (const char* why = svt::classify::take_arguments(text, len, n_samples, male, female, excluded, format_table, format_len, skip,
                                                            slope_threshold, rsquared_threshold, results, n_lines, info, b))
            return fail(SVT_ERR_INVALID, why);
        std::vector<svt_tbx_line> table;
        if (const char* why = svt::classify::classify_host(b, table, results, capacity, n_lines, *info)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

int svt_vcf_classify_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                           const uint8_t* format_table, uint64_t format_len, const svt_classify_line* results, uint64_t n_lines, uint64_t* out_off,
                           svt_classify_info* info)
{
    return cohort_write<svt::classify::Block>(text, len, n_samples, info_table, info_len, format_table, format_len, results, n_lines, out_off, info);
}

int svt_vcf_classify_take(uint8_t* out, uint64_t capacity) { return cohort_take<svt::classify::Block, svt_classify_line>(out, capacity); }

}  // extern "C"

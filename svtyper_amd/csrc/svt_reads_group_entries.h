// svt_reads_group_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// host entry points of svt_vcf_group.h: the records and the plan on the host, and the writer of the output text that both engines'
// plans go through (cohort_write with group::write_plan for its writing step, and cohort_take: svt_reads_cohort_entries.h); the
// device's entry is in svt_entry_vcf_group.h.
extern "C" {

int svt_vcf_group_host(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len, svt_group_line* lines,
                       uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan, svt_group_report* report)
{
    return guarded([&]() -> int {
        svt::group::Block b;
        if (const char* why = svt::group::take_arguments(text, len, n_samples, format_table, format_len, lines, n_lines, plan, n_plan, report, b))
            return fail(SVT_ERR_INVALID, why);
        if (const char* why = svt::group::group_host(b, lines, capacity, n_lines, plan, n_plan, *report)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

int svt_vcf_group_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len,
                        const uint8_t* format_table, uint64_t format_len, const svt_group_line* lines, uint64_t n_lines, const svt_group_out* plan,
                        uint64_t n_plan, uint64_t* out_off, svt_group_report* report)
{
    return cohort_write<svt::group::Block>(text, len, n_samples, info_table, info_len, format_table, format_len, lines, n_lines, out_off, report,
                                           [&](svt::group::Block& b, std::string& out, svt_group_report& r) {
                                               return svt::group::write_plan(b, lines, n_lines, plan, n_plan, out_off, out, r);
                                           },
                                           plan || !n_plan);
}

int svt_vcf_group_take(uint8_t* out, uint64_t capacity) { return cohort_take<svt::group::Block, svt_group_line>(out, capacity); }

}  // extern "C"

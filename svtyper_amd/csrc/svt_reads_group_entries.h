// svt_reads_group_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// host entry points of svt_vcf_group.h: the records and the plan on the host, and the writer of the output text that both engines'
// plans go through (_write leaves the text with the calling thread, _take copies it out, as svt_reads_cohort_entries.h does for
// the per-line rules); the device's entry is in svt_entry_vcf_group.h.
namespace {
std::string& group_text()
{
    thread_local std::string text;
    return text;
}
}  // namespace

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
    return guarded([&]() -> int {
        if (!report || !out_off || !format_table || (len && !text) || (n_lines && !lines) || (n_plan && !plan) || (info_len && !info_table))
            return fail(SVT_ERR_INVALID, "null argument");
        *report = svt_group_report();
        svt::group::Block b;
        if (len > svt::cohort::kMaxLine) return fail(SVT_ERR_INVALID, "svt_vcf_group: the body holds less than 2^31 bytes");
        if (!svt::cohort::parse_format_table(format_table, format_len, b.formats) || !svt::cohort::parse_info_table(info_table, info_len, b.info))
            return fail(SVT_ERR_INVALID, "svt_vcf_group_write: format_table is \"<id>\\n\" per id, info_table \"V<id>\\n\" or \"F<id>\\n\"");
        b.text = text;
        b.len = len;
        b.pr.n_samples = n_samples;
        if (const char* why = svt::group::write_plan(b, lines, n_lines, plan, n_plan, out_off, group_text(), *report)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

int svt_vcf_group_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&]() -> int {
        std::string& kept = group_text();
        if (capacity < kept.size() || (!out && !kept.empty())) return fail(SVT_ERR_INVALID, "svt_vcf_group_take: capacity is below the text");
        if (!kept.empty()) std::memcpy(out, kept.data(), kept.size());
        std::string().swap(kept);
        return SVT_OK;
    });
}

}  // extern "C"

// svt_reads_update_info_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone
// header): the host entry points of svt_vcf_update_info.h: the records on the host, and the writer of the output text that both
// engines' records go through; the device's entry is in svt_entry_vcf_update_info.h.
namespace {
thread_local std::string g_update_info_text;       // svt_vcf_update_info_write's, until svt_vcf_update_info_take
}

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
    return guarded([&]() -> int {
        if (!info || !out_off || !format_table || (len && !text) || (n_lines && !results) || (info_len && !info_table))
            return fail(SVT_ERR_INVALID, "null argument");
        *info = svt_update_info_report();
        svt::update_info::Block b;
        if (len > svt::paste::kMaxLine) return fail(SVT_ERR_INVALID, "svt_vcf_update_info: a block holds less than 2^31 bytes");
        if (!svt::classify::parse_format_table(format_table, format_len, b.formats) || !svt::paste::parse_info_table(info_table, info_len, b.info))
            return fail(SVT_ERR_INVALID, "svt_vcf_update_info_write: format_table is \"<id>\\n\" per id, info_table \"V<id>\\n\" or \"F<id>\\n\"");
        b.text = text;
        b.len = len;
        b.pr.n_samples = n_samples;
        std::vector<svt_tbx_line> table;
        if (const char* why = svt::update_info::write_block(b, table, results, n_lines, out_off, g_update_info_text, *info))
            return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

int svt_vcf_update_info_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&]() -> int {
        if (capacity < g_update_info_text.size() || (!out && !g_update_info_text.empty()))
            return fail(SVT_ERR_INVALID, "svt_vcf_update_info_take: capacity is below the text");
        if (!g_update_info_text.empty()) std::memcpy(out, g_update_info_text.data(), g_update_info_text.size());
        std::string().swap(g_update_info_text);
        return SVT_OK;
    });
}

}  // extern "C"

// svt_reads_paste_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// host entry point over per-sample VCFs joined by line number (svt_vcf_paste.h); the device's is in svt_entry_vcf_paste.h.
extern "C" {

int svt_vcf_paste_host(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines, uint32_t flags,
                       const uint8_t* info_table, uint64_t info_len, uint8_t* out, uint64_t capacity, svt_paste_line* results, svt_paste_info* info)
{
    return guarded([&]() -> int {
        svt::paste::Block b;
        if (const char* why = svt::paste::take_arguments(text, len, first_line, n_inputs, n_lines, flags, info_table, info_len, out, results, info, b))
            return fail(SVT_ERR_INVALID, why);
        std::vector<svt_tbx_line> table;
        if (const char* why = svt::paste::paste_host(b, table, results, out, capacity, *info)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

}  // extern "C"

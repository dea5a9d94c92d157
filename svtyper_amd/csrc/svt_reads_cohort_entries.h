// svt_reads_cohort_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header):
// the writer's two entry points of a rule over cohort lines (svt_vcf_cohort_line.h), once for svt_reads_classify_entries.h,
// svt_reads_update_info_entries.h and svt_reads_group_entries.h: _write leaves the output text with the calling thread, _take
// copies it out.
namespace {

template <class Line>
std::string& cohort_text()                          // the thread's text of the rule whose records are Line, from _write until _take
{
    thread_local std::string text;
    return text;
}

// write(b, out, info) is the rule's writing step over the block b into the thread's text: what is wrong with the call, or nullptr.
// `others`: the pointers that are the rule's alone are there
template <class Block, class Line, class Info, class Write>
int cohort_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len, const uint8_t* format_table,
                 uint64_t format_len, const Line* results, uint64_t n_lines, uint64_t* out_off, Info* info, Write write, bool others = true)
{
    return guarded([&]() -> int {
        const std::string name = Block::kName;
        if (!info || !out_off || !format_table || (len && !text) || (n_lines && !results) || !others || (info_len && !info_table))
            return fail(SVT_ERR_INVALID, "null argument");
        *info = Info();
        Block b;
        if (len > svt::cohort::kMaxLine) return fail(SVT_ERR_INVALID, Block::kLengthWhy);
        if (!svt::cohort::parse_format_table(format_table, format_len, b.formats) || !svt::cohort::parse_info_table(info_table, info_len, b.info))
            return fail(SVT_ERR_INVALID, name + "_write: format_table is \"<id>\\n\" per id, info_table \"V<id>\\n\" or \"F<id>\\n\"");
        b.text = text;
        b.len = len;
        b.pr.n_samples = n_samples;
        if (const char* why = write(b, cohort_text<Line>(), *info)) return fail(SVT_ERR_INVALID, why);
        return SVT_OK;
    });
}

// the writing step of a rule over single lines: one record per line (cohort::write_block)
template <class Block, class Line, class Info>
int cohort_write(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* info_table, uint64_t info_len, const uint8_t* format_table,
                 uint64_t format_len, const Line* results, uint64_t n_lines, uint64_t* out_off, Info* info)
{
    return cohort_write<Block>(text, len, n_samples, info_table, info_len, format_table, format_len, results, n_lines, out_off, info,
                               [&](Block& b, std::string& out, Info& report) {
                                   std::vector<svt_tbx_line> table;
                                   return svt::cohort::write_block(b, table, results, n_lines, out_off, out, report);
                               });
}

template <class Block, class Line>
int cohort_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&]() -> int {
        std::string& kept = cohort_text<Line>();
        if (capacity < kept.size() || (!out && !kept.empty())) return fail(SVT_ERR_INVALID, std::string(Block::kName) + "_take: capacity is below the text");
        if (!kept.empty()) std::memcpy(out, kept.data(), kept.size());
        std::string().swap(kept);
        return SVT_OK;
    });
}

}  // namespace

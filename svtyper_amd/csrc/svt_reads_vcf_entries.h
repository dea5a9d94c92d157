// svt_reads_vcf_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// host entry points over VCF text as lines (svt_vcf_lines.h) and the index fold (svt_tbx_index.h); and what that fold's entries share
// with the .bai fold's (svt_reads_bam_sort_entries.h): the result holder and the check of member_off.
namespace {

// An index built into a thread-local buffer by a *_build entry, which reports its size; the *_take entry hands it over once and frees it.
struct HeldResult {
    std::vector<uint8_t> bytes;
    template <typename Fill> void build(uint64_t* size, Fill&& fill) { bytes.clear(); *size = 0; fill(bytes); *size = bytes.size(); }
    int take(const char* entry, uint8_t* out, uint64_t capacity)
    {
        if (bytes.size() > capacity || (!out && !bytes.empty())) return fail(SVT_ERR_INVALID, std::string(entry) + ": capacity is below the result");
        if (!bytes.empty()) std::memcpy(out, bytes.data(), bytes.size());
        std::vector<uint8_t>().swap(bytes);
        return SVT_OK;
    }
};

// member_off[0 .. n_members]: where the members begin in the file, as virtual offsets can say it
int check_member_off(const char* entry, const uint64_t* member_off, uint64_t n_members)
{
    for (uint64_t k = 0; k < n_members; ++k)
        if (member_off[k + 1] < member_off[k] || member_off[k + 1] >> 48) return fail(SVT_ERR_INVALID, std::string(entry) + ": member_off must not decrease (< 2^48)");
    return SVT_OK;
}

// what svt_tbx_build and svt_csi_build_vcf ask of their tables, in the entry's name
int check_line_table(const char* entry, uint64_t len, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n, const uint64_t* member_off,
                     uint64_t n_members, uint32_t payload)
{
    const std::string who(entry);
    if (payload < 1 || payload > 65536) return fail(SVT_ERR_INVALID, who + ": a payload has 1 .. 65536 bytes");
    if (len > n_members * (uint64_t)payload) return fail(SVT_ERR_INVALID, who + ": the members hold less than the text");
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {            // the table of a text as written: the lines side by side
        if (lines[i].off != at || lines[i].len > len - at) return fail(SVT_ERR_INVALID, who + ": the lines do not tile the text");
        const uint64_t src = src_off ? src_off[i] : lines[i].off;
        if (src > len || lines[i].chrom_len > len - src) return fail(SVT_ERR_INVALID, who + ": a CHROM lies outside the text");
        at += lines[i].len;
    }
    return check_member_off(entry, member_off, n_members);
}

}  // namespace

extern "C" {

int svt_vcf_lines_host(const uint8_t* text, uint64_t len, svt_tbx_line* lines, uint64_t capacity, uint64_t* n_lines)
{
    return guarded([&]() -> int {
        if (!n_lines || (len && !text)) return fail(SVT_ERR_INVALID, "null argument");
        *n_lines = svt::tbx::count_lines(text, len);
        if (*n_lines > capacity) return fail(SVT_ERR_INVALID, "svt_vcf_lines: capacity is below the number of lines");
        if (*n_lines && !lines) return fail(SVT_ERR_INVALID, "null argument");
        svt::tbx::lines_host(text, len, lines);
        return SVT_OK;
    });
}

int svt_vcf_gather_host(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm, uint64_t n_perm,
                        uint8_t* out, uint64_t out_len)
{
    return guarded([&]() -> int {
        if ((len && !text) || (n && !lines) || (n_perm && !perm) || (out_len && !out)) return fail(SVT_ERR_INVALID, "null argument");
        std::vector<uint64_t> dst_off;
        if (const char* why = svt::tbx::gather_plan(len, lines, n, perm, n_perm, out_len, dst_off)) return fail(SVT_ERR_INVALID, why);
        svt::tbx::gather_host(text, lines, perm, n_perm, dst_off.data(), out);
        return SVT_OK;
    });
}

int svt_vcf_sort_order(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, uint64_t* perm, uint64_t* bad_line)
{
    return guarded([&]() -> int {
        if ((len && !text) || (n && (!lines || !perm)) || !bad_line) return fail(SVT_ERR_INVALID, "null argument");
        for (uint64_t i = 0; i < n; ++i)
            if (lines[i].off > len || lines[i].len > len - lines[i].off) return fail(SVT_ERR_INVALID, "svt_vcf_sort_order: a line lies outside the text");
        *bad_line = svt::tbx::sort_order(text, lines, n, perm);
        return SVT_OK;
    });
}

static thread_local HeldResult g_tbx_result;

int svt_tbx_build(const uint8_t* text, uint64_t len, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n, const uint64_t* member_off,
                  uint64_t n_members, uint32_t payload, uint64_t* size, uint64_t* bad_line, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((len && !text) || (n && !lines) || !member_off || !size || !bad_line || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (const int rc = check_line_table("svt_tbx_build", len, src_off, lines, n, member_off, n_members, payload)) return rc;
        *bad_kind = 0;
        g_tbx_result.build(size, [&](std::vector<uint8_t>& tbi) {
            *bad_line = svt::tbx::build(text, src_off, lines, n, len, member_off, n_members, payload, tbi, *bad_kind);
        });
        return SVT_OK;
    });
}

int svt_tbx_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&] { return g_tbx_result.take("svt_tbx_take", out, capacity); });
}

}  // extern "C"

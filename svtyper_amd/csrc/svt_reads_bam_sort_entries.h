// svt_reads_bam_sort_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header):
// the host entry points over BAM records as spans (svt_bam_sort_rules.h), the .bai fold (svt_bai_index.h) and the first occurrences
// of a record stream (svt_bam_first_rules.h).
extern "C" {

int svt_bam_spans_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, svt_bam_span* spans, uint64_t* key_and,
                       uint64_t* key_or)
{
    return guarded([&]() -> int {
        if ((len && !bytes) || !rec_off || (n && !spans)) return fail(SVT_ERR_INVALID, "null argument");
        if (n_ref < 0) return fail(SVT_ERR_INVALID, "svt_bam_spans: n_ref is negative");
        uint64_t a = ~0ull, o = 0;
        svt::bsr::spans_host(bytes, len, rec_off, n, n_ref, spans, a, o);
        if (key_and) *key_and = a;
        if (key_or) *key_or = o;
        return SVT_OK;
    });
}

int svt_bam_sort_order_host(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((n && (!spans || !perm)) || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_sort_order: too many records in one call (< 2^32)");
        *bad_record = svt::bsr::sort_order(spans, n, perm, *bad_kind);
        return SVT_OK;
    });
}

int svt_bam_first_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept, uint64_t* bad_record)
{
    return guarded([&]() -> int {
        if ((len && !bytes) || !rec_off || (n && !keep) || !n_kept || !bad_record) return fail(SVT_ERR_INVALID, "null argument");
        if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_first: too many records in one call (< 2^32)");
        for (uint64_t i = 0; i < n; ++i)
            if (rec_off[i] > rec_off[i + 1]) return fail(SVT_ERR_INVALID, "svt_bam_first: rec_off must not decrease");
        *bad_record = svt::bfr::first_host(bytes, len, rec_off, n, keep, *n_kept);
        return SVT_OK;
    });
}

static thread_local HeldResult g_bai_result;            // (svt_reads_vcf_entries.h)
static thread_local HeldResult g_csi_result;            // svt_csi_build_bam, svt_csi_build_vcf and the device fold (svt_entry_bam_index.h)

// what svt_bai_build and svt_csi_build_bam ask of their tables (bai::check_tables), in the entry's name
static int check_span_table(const char* entry, const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start,
                            const uint64_t* member_off, uint64_t n_members)
{
    if (const char* why = svt::bai::check_tables(spans, n, n_ref, l_ref_max, member_start, member_off, n_members))
        return fail(SVT_ERR_INVALID, std::string(entry) + ": " + why);
    return SVT_OK;
}

int svt_bai_build(const svt_bam_span* spans, uint64_t n, int32_t n_ref, const uint64_t* member_start, const uint64_t* member_off, uint64_t n_members,
                  uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((n && !spans) || !member_start || !member_off || !size || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (const int rc = check_span_table("svt_bai_build", spans, n, n_ref, 0, member_start, member_off, n_members)) return rc;
        *bad_kind = 0;
        g_bai_result.build(size, [&](std::vector<uint8_t>& bai) {
            *bad_record = svt::bai::build(spans, n, n_ref, member_start, member_off, n_members, bai, *bad_kind);
        });
        return SVT_OK;
    });
}

int svt_bai_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&] { return g_bai_result.take("svt_bai_take", out, capacity); });
}

uint32_t svt_csi_depth(uint64_t max_end) { return svt::idx::depth_for(max_end); }

int svt_csi_build_bam(const svt_bam_span* spans, uint64_t n, int32_t n_ref, uint64_t l_ref_max, const uint64_t* member_start, const uint64_t* member_off,
                      uint64_t n_members, uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((n && !spans) || !member_start || !member_off || !size || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (const int rc = check_span_table("svt_csi_build_bam", spans, n, n_ref, l_ref_max, member_start, member_off, n_members)) return rc;
        *bad_kind = 0;
        g_csi_result.build(size, [&](std::vector<uint8_t>& csi) {
            *bad_record = svt::bai::build(spans, n, n_ref, member_start, member_off, n_members, csi, *bad_kind, true, l_ref_max);
        });
        return SVT_OK;
    });
}

int svt_csi_build_vcf(const uint8_t* text, uint64_t len, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n, const uint64_t* member_off,
                      uint64_t n_members, uint32_t payload, uint64_t* size, uint64_t* bad_line, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((len && !text) || (n && !lines) || !member_off || !size || !bad_line || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (const int rc = check_line_table("svt_csi_build_vcf", len, src_off, lines, n, member_off, n_members, payload)) return rc;
        *bad_kind = 0;
        g_csi_result.build(size, [&](std::vector<uint8_t>& csi) {
            *bad_line = svt::tbx::build(text, src_off, lines, n, len, member_off, n_members, payload, csi, *bad_kind, true);
        });
        return SVT_OK;
    });
}

int svt_csi_take(uint8_t* out, uint64_t capacity)
{
    return guarded([&] { return g_csi_result.take("svt_csi_take", out, capacity); });
}

}  // extern "C"

// where the device fold (svtyper_hip.hip: svt_entry_bam_index.h) leaves its bytes for svt_csi_take: the calling thread's held result
namespace svt {
std::vector<uint8_t>& csi_held_bytes() { return g_csi_result.bytes; }
}  // namespace svt

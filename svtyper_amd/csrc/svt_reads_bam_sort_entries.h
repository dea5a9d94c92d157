// svt_reads_bam_sort_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header):
// the host entry points over BAM records as spans (svt_bam_sort_rules.h) and the .bai fold (svt_bai_index.h).
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

static thread_local HeldResult g_bai_result;            // (svt_reads_vcf_entries.h)

int svt_bai_build(const svt_bam_span* spans, uint64_t n, int32_t n_ref, const uint64_t* member_start, const uint64_t* member_off, uint64_t n_members,
                  uint64_t* size, uint64_t* bad_record, uint32_t* bad_kind)
{
    return guarded([&]() -> int {
        if ((n && !spans) || !member_start || !member_off || !size || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
        if (n_ref < 0) return fail(SVT_ERR_INVALID, "svt_bai_build: n_ref is negative");
        for (uint64_t k = 0; k < n_members; ++k)
            if (member_start[k + 1] < member_start[k] || member_start[k + 1] - member_start[k] > 65536)
                return fail(SVT_ERR_INVALID, "svt_bai_build: member_start must not decrease, a member holds at most 65536 bytes");
        if (const int rc = check_member_off("svt_bai_build", member_off, n_members)) return rc;
        uint64_t at = n ? spans[0].off : 0;
        if (n && at < member_start[0]) return fail(SVT_ERR_INVALID, "svt_bai_build: a record lies in front of the members");
        for (uint64_t i = 0; i < n; ++i) {            // the table of a stream as written: the records side by side
            if (spans[i].off != at || spans[i].len > member_start[n_members] - at) return fail(SVT_ERR_INVALID, "svt_bai_build: the records do not tile the stream");
            at += spans[i].len;
        }
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

}  // extern "C"

// svt_reads_bcf_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// host entry points over VCF text as a BCF stream (svt_bcf.h) and back (svt_bcf_text.h), and the results the device entries
// (svtyper_hip.hip: svt_entry_bcf.h, svt_entry_bcf_text.h) share with them.
static thread_local svt::bcf::Held g_bcf_held;
static thread_local svt::bcftext::TextHeld g_bcf_text_held;

extern "C" {

int svt_bcf_encode_host(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info)
{
    return guarded([&]() -> int {
        if (!info || (len && !text)) return fail(SVT_ERR_INVALID, "null argument");
        if (flags & ~(SVT_BCF_SORT | SVT_BCF_EXACT_FLOATS)) return fail(SVT_ERR_INVALID, "svt_bcf_encode: flags are SVT_BCF_SORT and SVT_BCF_EXACT_FLOATS");
        *info = svt_bcf_info();
        g_bcf_held.clear();
        if (const char* why = svt::bcf::encode_host(text, len, (flags & SVT_BCF_SORT) != 0, (flags & SVT_BCF_EXACT_FLOATS) != 0, *info, g_bcf_held)) {
            g_bcf_held.clear();
            return fail(SVT_ERR_INVALID, std::string("svt_bcf_encode: ") + why);
        }
        if (info->bad_line) g_bcf_held.clear();
        info->bytes_len = info->stream_len = g_bcf_held.bytes.size();
        info->n_offsets = g_bcf_held.offsets.size();
        return SVT_OK;
    });
}

int svt_bcf_take(uint8_t* bytes, uint64_t bytes_capacity, uint64_t* offsets, uint64_t offsets_capacity, uint64_t* starts, svt_bam_span* spans,
                 uint64_t spans_capacity)
{
    return guarded([&]() -> int {
        svt::bcf::Held& h = g_bcf_held;
        if (h.bytes.size() > bytes_capacity || h.offsets.size() > offsets_capacity || h.spans.size() > spans_capacity)
            return fail(SVT_ERR_INVALID, "svt_bcf_take: a capacity is below the result");
        if ((!bytes && !h.bytes.empty()) || (!offsets && !h.offsets.empty()) || (!spans && !h.spans.empty())) return fail(SVT_ERR_INVALID, "null argument");
        if (!h.bytes.empty()) std::memcpy(bytes, h.bytes.data(), h.bytes.size());
        if (!h.offsets.empty()) std::memcpy(offsets, h.offsets.data(), h.offsets.size() * sizeof(uint64_t));
        if (starts && !h.starts.empty()) std::memcpy(starts, h.starts.data(), h.starts.size() * sizeof(uint64_t));
        if (!h.spans.empty()) std::memcpy(spans, h.spans.data(), h.spans.size() * sizeof(svt_bam_span));
        h.clear();
        return SVT_OK;
    });
}

int svt_bcf_text_host(const uint8_t* stream, uint64_t len, uint32_t flags, uint64_t block_bytes, svt_bcf_text_info* info)
{
    return guarded([&]() -> int {
        if (!info || (len && !stream)) return fail(SVT_ERR_INVALID, "null argument");
        if (flags & ~SVT_BCF_TEXT_EXACT_FLOATS) return fail(SVT_ERR_INVALID, "svt_bcf_text: the only flag is SVT_BCF_TEXT_EXACT_FLOATS");
        *info = svt_bcf_text_info();
        g_bcf_text_held.clear();
        const char* why = svt::bcftext::text_host(stream, len, (flags & SVT_BCF_TEXT_EXACT_FLOATS) != 0, block_bytes ? block_bytes : ~0ull, *info,
                                                  g_bcf_text_held);
        if (why || info->bad_record) g_bcf_text_held.clear();
        if (why) return fail(SVT_ERR_INVALID, std::string("svt_bcf_text: ") + why);
        info->text_len = g_bcf_text_held.text.size();
        info->n_offsets = g_bcf_text_held.offsets.size();
        return SVT_OK;
    });
}

int svt_bcf_text_take(uint8_t* text, uint64_t text_capacity, uint64_t* offsets, uint64_t offsets_capacity, uint8_t* marks, uint64_t marks_capacity)
{
    return guarded([&]() -> int {
        svt::bcftext::TextHeld& h = g_bcf_text_held;
        if (h.text.size() > text_capacity || h.offsets.size() > offsets_capacity || h.marks.size() > marks_capacity)
            return fail(SVT_ERR_INVALID, "svt_bcf_text_take: a capacity is below the result");
        if ((!text && !h.text.empty()) || (!offsets && !h.offsets.empty()) || (!marks && !h.marks.empty())) return fail(SVT_ERR_INVALID, "null argument");
        if (!h.text.empty()) std::memcpy(text, h.text.data(), h.text.size());
        if (!h.offsets.empty()) std::memcpy(offsets, h.offsets.data(), h.offsets.size() * sizeof(uint64_t));
        if (!h.marks.empty()) std::memcpy(marks, h.marks.data(), h.marks.size());
        h.clear();
        return SVT_OK;
    });
}

}  // extern "C"

// where the device entries leave their results for svt_bcf_take and svt_bcf_text_take: the calling thread's
namespace svt {
namespace bcf {
Held& held_result() { return g_bcf_held; }
}  // namespace bcf
namespace bcftext {
TextHeld& held_result() { return g_bcf_text_held; }
}  // namespace bcftext
}  // namespace svt

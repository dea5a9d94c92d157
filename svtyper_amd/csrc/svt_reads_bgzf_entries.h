// svt_reads_bgzf_entries.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the
// stand-alone BGZF entry points on the host: inflate (plain and verified), CRC-32, deflate.  Needs: bgzf_members,
// inflate_members_host (svt_bgzf_reader.h).
extern "C" {

static int svt_bgzf_inflate_host_impl(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                      const uint64_t* out_off, uint32_t* status, bool verify)
{
    svt::bgzf::MemberSet set;
    if (const int rc = svt::bgzf::bgzf_members(data, len, block_off, n, out, out_off, status, set)) return rc;
    // (the one-source decoder and CRC on this thread, as the device entry's kernels run them; nothing is counted)
    svt::VerifyTally uncounted;
    std::vector<uint32_t> st;
    svt::bgzf::inflate_members_host(set, out, 1, svt::bgzf::Decoder::one_source, svt::bgzf::Crc::one_source, verify ? &uncounted : nullptr, st);
    if (n) std::memcpy(status, st.data(), n * sizeof(uint32_t));
    return SVT_OK;
}

int svt_bgzf_inflate_host(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out, const uint64_t* out_off,
                          uint32_t* status)
{
    return guarded([&] { return svt_bgzf_inflate_host_impl(data, len, block_off, n, out, out_off, status, false); });
}

int svt_bgzf_inflate_host_verified(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                   const uint64_t* out_off, uint32_t* status)
{
    return guarded([&] { return svt_bgzf_inflate_host_impl(data, len, block_off, n, out, out_off, status, true); });
}

int svt_bgzf_crc32_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t* crc)
{
    return guarded([&]() -> int {
        if (const int rc = svt::crc_check_offsets(bytes, off, n, crc)) return rc;
        std::unique_ptr<svt::crc::Scratch> C(new svt::crc::Scratch());
        for (uint64_t k = 0; k < n; ++k) crc[k] = svt::crc::crc_member<svt::crc::HostCtx>(bytes + off[k], (uint32_t)(off[k + 1] - off[k]), svt::crc_tables(), *C);
        return SVT_OK;
    });
}

// svt_deflate.h on this thread, member by member: each into a slot of its own first, since its size is known only afterwards
extern "C++" {
template <uint32_t M>
static int svt_bgzf_deflate_host_impl(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off)
{
    namespace dfl = svt::dfl;
    uint64_t slots = 0;
    if (const int rc = svt::deflate_check_args(bytes, off, n, out, out_off, slots)) return rc;
    std::unique_ptr<dfl::Scratch<dfl::HostCtx::kWidth, M>> S(new dfl::Scratch<dfl::HostCtx::kWidth, M>());
    std::unique_ptr<svt::crc::Scratch> C(new svt::crc::Scratch());
    std::vector<uint8_t> slot(dfl::slot_bytes(dfl::kMaxPayload));
    uint64_t at = 0;
    out_off[0] = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint8_t* p = bytes + off[k];
        const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
        const uint32_t clen = dfl::deflate_member<dfl::HostCtx, M>(p, len, slot.data() + dfl::kHeaderBytes, dfl::cdata_bound(len), *S);
        if (!clen) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: a payload was refused");
        const uint64_t size = (uint64_t)dfl::kHeaderBytes + clen + dfl::kTrailerBytes;
        if (size > capacity - at) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: capacity is below what the members need");
        const uint32_t crc = svt::crc::crc_member<svt::crc::HostCtx>(p, len, svt::crc_tables(), *C);
        for (uint32_t i = 0; i < dfl::kHeaderBytes; ++i) slot[i] = dfl::header_byte(i, clen);
        for (uint32_t i = 0; i < dfl::kTrailerBytes; ++i) slot[dfl::kHeaderBytes + clen + i] = dfl::trailer_byte(i, crc, len);
        std::memcpy(out + at, slot.data(), size);
        at += size;
        out_off[k + 1] = at;
    }
    return SVT_OK;
}
}  // extern "C++"

int svt_bgzf_deflate_host(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off)
{
    return guarded([&] { return svt_bgzf_deflate_host_impl<svt::dfl::kFixed>(bytes, off, n, out, capacity, out_off); });
}

int svt_bgzf_deflate_host_mode(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint32_t mode)
{
    return guarded([&]() -> int {
        if (mode == SVT_DEFLATE_FIXED) return svt_bgzf_deflate_host_impl<svt::dfl::kFixed>(bytes, off, n, out, capacity, out_off);
        if (mode == SVT_DEFLATE_DYNAMIC) return svt_bgzf_deflate_host_impl<svt::dfl::kDynamic>(bytes, off, n, out, capacity, out_off);
        return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: mode is SVT_DEFLATE_FIXED (0) or SVT_DEFLATE_DYNAMIC (1)");
    });
}

// dfl::code_lengths on this thread, histogram by histogram
int svt_huffman_lengths_host(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, uint8_t* lengths)
{
    namespace dfl = svt::dfl;
    return guarded([&]() -> int {
        if (const int rc = svt::huffman_check_args(freq, sets, symbols, limit, lengths)) return rc;
        std::unique_ptr<dfl::Build> B(new dfl::Build());
        for (uint64_t k = 0; k < sets; ++k) dfl::code_lengths<dfl::HostCtx>(freq + k * symbols, symbols, limit, lengths + k * symbols, *B);
        return SVT_OK;
    });
}

}  // extern "C"

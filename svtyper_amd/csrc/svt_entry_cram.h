// svt_entry_cram.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the host
// entry points of the CRAM reader.  svt_rans_decode_host: a batch of rANS 4x8 blocks by the one-source decoder of svt_rans.h, the
// blocks shared among the host's threads.  svt_cram_decode_slice / svt_cram_take: one slice as BAM records (svt_cram.h), left
// for the calling thread to take.  C ABI: include/svtyper_reads.h.
extern "C" {

int svt_rans_decode_host(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off, const uint64_t* out_size,
                         uint8_t* out, uint64_t out_len, uint32_t* status)
{
    namespace rans = svt::rans;
    return guarded([&]() -> int {
        std::vector<rans::Job> order0, order1;
        if (const int rc = rans::plan_batch(data, data_len, off, n, out_off, out_size, out, out_len, status, order0, order1)) return rc;
        const size_t jobs = order0.size() + order1.size();
        if (!jobs) return SVT_OK;
        const unsigned nt = (unsigned)std::min<size_t>(svt::usable_cpus(), jobs);
        run_threads(nt, [&](unsigned t) {
            std::vector<uint16_t> C;
            for (size_t k = t; k < jobs; k += nt) {
                const bool one = k >= order0.size();
                const rans::Job& j = one ? order1[k - order0.size()] : order0[k];
                C.assign(one ? (size_t)256 * rans::kCtx : (size_t)rans::kCtx, 0);
                const uint32_t st = rans::decode_serial(one, data + j.in_off, j.in_len, out + j.out_off, j.out_len, C.data());
                if (st != rans::RANS_OK) rans::zero_out(out + j.out_off, j.out_len);
                status[j.block] = st;
            }
        });
        return SVT_OK;
    });
}

extern "C++" {
namespace {
struct CramHeld {
    std::vector<uint8_t> records;
    std::vector<uint64_t> rec_off;
    void clear()
    {
        records.clear();
        rec_off.clear();
    }
};
CramHeld& cram_held()
{
    static thread_local CramHeld held;
    return held;
}
}  // namespace
}  // extern "C++"

int svt_cram_decode_slice(const uint8_t* comp_header, uint64_t comp_len, const uint8_t* slice_header, uint64_t slice_len, const uint8_t* blocks,
                          const uint64_t* block_off, const int32_t* content_id, const uint8_t* is_core, uint32_t n_blocks, const char* rg_ids, uint32_t n_rg,
                          int32_t n_ref, svt_cram_slice_info* info)
{
    namespace cram = svt::cram;
    return guarded([&]() -> int {
        CramHeld& held = cram_held();
        held.clear();
        if (!info || !comp_header || !slice_header || (n_blocks && (!block_off || !content_id || !is_core)) || (n_rg && !rg_ids))
            return fail(SVT_ERR_INVALID, "svt_cram_decode_slice: null argument");
        *info = svt_cram_slice_info();
        std::vector<cram::Block> bl(n_blocks);
        for (uint32_t k = 0; k < n_blocks; ++k) {
            if (block_off[k + 1] < block_off[k]) return fail(SVT_ERR_INVALID, "svt_cram_decode_slice: block_off must rise");
            bl[k] = cram::Block{blocks + block_off[k], (size_t)(block_off[k + 1] - block_off[k]), content_id[k], is_core[k] != 0};
        }
        std::vector<std::string> rg(n_rg);
        const char* p = rg_ids;
        for (uint32_t k = 0; k < n_rg; ++k) {
            rg[k] = p;
            p += rg[k].size() + 1;
        }
        try {
            cram::decode_slice(comp_header, comp_len, slice_header, slice_len, bl, rg, n_ref, held.records, held.rec_off);
        } catch (const cram::Refuse& e) {
            held.clear();
            return fail(SVT_ERR_INVALID, e.what());
        }
        info->n_records = held.rec_off.size() - 1;
        info->bytes = held.records.size();
        return SVT_OK;
    });
}

int svt_cram_take(uint8_t* records, uint64_t* rec_off)
{
    return guarded([&]() -> int {
        CramHeld& held = cram_held();
        if (held.rec_off.empty()) return fail(SVT_ERR_INVALID, "svt_cram_take: no decoded slice is held");
        if (!rec_off || (!records && !held.records.empty())) return fail(SVT_ERR_INVALID, "null argument");
        if (!held.records.empty()) std::memcpy(records, held.records.data(), held.records.size());
        std::memcpy(rec_off, held.rec_off.data(), held.rec_off.size() * sizeof(uint64_t));
        held.clear();
        return SVT_OK;
    });
}

}  // extern "C"

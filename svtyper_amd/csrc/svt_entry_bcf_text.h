// svt_entry_bcf_text.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind svt_entry_bcf.h;
// not a stand-alone header): an inflated BCF stream as VCF text on the device.  What is this header's: the header and the record
// chain on the host (svt_bcf_text.h: read_stream_header, walk_chain), the dictionaries' upload, and per chunk of at most
// block_bytes of stream the upload, the two launches of svt_bcf_text_kernel.h around the host's prefix sum, the download, and
// the lines the host twin writes for the records outside the float envelope; the result left for svt_bcf_text_take.
// C ABI: svt_bcf_text_device, svt_bcf_text_last_times (include/svtyper_bcf.h).

extern "C++" {

namespace svt {
namespace bcftext {
TextHeld& held_result();                            // (svt_reads.cpp: the calling thread's result for svt_bcf_text_take)
}
}

// the kernels and copies of the calling thread's last call here, from HIP events, and the call's wall time
static thread_local svt_bcf_text_times g_bcf_text_times;

struct BcfTextCall : TimedCallStream {                       // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_dict, d_stream, d_rec_off, d_measures, d_text_off, d_text;
    ~BcfTextCall() { drain(); }
};

// the tables of `t` side by side in one allocation; the view over them
static int upload_text_dict(BcfTextCall& c, const bcftext::TextTables& t, bcftext::TextDict& d)
{
    std::vector<uint8_t> blob;
    auto add = [&](const void* p, size_t bytes) {
        const size_t at = blob.size();
        blob.insert(blob.end(), (const uint8_t*)p, (const uint8_t*)p + bytes);
        blob.resize((blob.size() + 15) & ~(size_t)15);
        return at;
    };
    const size_t name_off = add(t.name_off.data(), t.name_off.size() * 4), cname_off = add(t.cname_off.data(), t.cname_off.size() * 4);
    const size_t names = add(t.names.data(), t.names.size()), types = add(t.types.data(), t.types.size());
    const size_t cnames = add(t.cnames.data(), t.cnames.size()), chave = add(t.chave.data(), t.chave.size());
    SVT_TRY(c.d_dict.alloc(blob.size()));
    SVT_TRY(h2d_staged(c.d_dict.p, blob.data(), blob.size(), c.s));
    const uint8_t* base = c.d_dict.as<uint8_t>();
    d = t.view();
    d.names = base + names;
    d.types = base + types;
    d.cnames = base + cnames;
    d.chave = base + chave;
    d.name_off = reinterpret_cast<const uint32_t*>(base + name_off);
    d.cname_off = reinterpret_cast<const uint32_t*>(base + cname_off);
    return SVT_OK;
}

static int svt_bcf_text_device_impl(const uint8_t* stream, uint64_t len, uint32_t flags, uint64_t block_bytes, svt_bcf_text_info* info, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!info || (len && !stream)) return fail(SVT_ERR_INVALID, "null argument");
    if (flags) return fail(SVT_ERR_INVALID, "svt_bcf_text: the device route takes no flag");
    *info = svt_bcf_text_info();
    g_bcf_text_times = svt_bcf_text_times();
    bcftext::TextHeld& held = bcftext::held_result();
    held.clear();
    SVT_TRY(select_device(device));
    bcftext::TextTables t;
    uint64_t body = 0;
    if (const char* why = bcftext::read_stream_header(stream, len, t, body)) return fail(SVT_ERR_INVALID, std::string("svt_bcf_text: ") + why);
    const bcftext::TextDict host_dict = t.view();
    std::vector<uint64_t> chain;
    const bool cut_short = bcftext::walk_chain(stream, len, body, chain);
    const uint64_t n = chain.size() - 1;
    if (!block_bytes) block_bytes = ~0ull;
    info->n_sample = t.n_sample;
    info->header_len = t.header.size();
    held.text.assign(t.header.begin(), t.header.end());
    held.offsets.assign(1, held.text.size());
    held.marks.assign(n, 0);
    // the largest chunk sizes the buffers the chunks share
    uint64_t most_bytes = 0, most_records = 0;
    for (uint64_t from = 0; from < n; ) {
        const uint64_t to = bcftext::chunk_end(chain, from, block_bytes);
        most_bytes = std::max(most_bytes, chain[to] - chain[from]);
        most_records = std::max(most_records, to - from);
        from = to;
    }
    BcfTextCall c;
    bcftext::TextDict d;
    uint64_t text_cap = 0;
    if (n) {
        SVT_TRY(c.take());
        SVT_TRY(upload_text_dict(c, t, d));
        SVT_TRY(c.d_stream.alloc(most_bytes));
        SVT_TRY(c.d_rec_off.alloc((most_records + 1) * sizeof(uint64_t)));
        SVT_TRY(c.d_text_off.alloc((most_records + 1) * sizeof(uint64_t)));
        SVT_TRY(c.d_measures.alloc(most_records * sizeof(bcftext::TextMeasure)));
    }
    std::vector<bcftext::TextMeasure> m;
    std::vector<uint64_t> rec_off, text_off;
    for (uint64_t from = 0; from < n; ++info->chunks) {
        const uint64_t to = bcftext::chunk_end(chain, from, block_bytes), k = to - from, bytes = chain[to] - chain[from];
        const uint8_t* chunk = stream + chain[from];
        rec_off.resize(k + 1);
        for (uint64_t j = 0; j <= k; ++j) rec_off[j] = chain[from + j] - chain[from];
        const unsigned grid = capped_grid((k + kBcfTextWaves - 1) / kBcfTextWaves, 8, device);
        size_t e[8] = {};
        SVT_TRY(c.mark(&e[0]));
        SVT_TRY(h2d_staged(c.d_stream.p, chunk, bytes, c.s));
        SVT_TRY(h2d_staged(c.d_rec_off.p, rec_off.data(), (k + 1) * sizeof(uint64_t), c.s));
        SVT_TRY(c.mark(&e[1]));
        hipLaunchKernelGGL(svt_bcf_text_measure_kernel, dim3(grid), dim3(kBcfTextBlock), 0, c.s, c.d_stream.as<uint8_t>(), bytes, c.d_rec_off.as<uint64_t>(), k,
                           d, c.d_measures.as<bcftext::TextMeasure>());
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[2]));
        m.resize(k);
        SVT_TRY(d2h_staged(m.data(), c.d_measures.p, k * sizeof(bcftext::TextMeasure), c.s));
        SVT_TRY(c.between(e[0], e[1], &g_bcf_text_times.upload_s));
        SVT_TRY(c.between(e[1], e[2], &g_bcf_text_times.measure_kernel_s));
        // the records outside the envelope: the host twin's lengths; the lowest refusal
        text_off.assign(k + 1, 0);
        for (uint64_t j = 0; j < k; ++j) {
            if (m[j].kind) {
                info->bad_record = from + j + 1;
                info->bad_kind = m[j].kind;
                held.clear();
                return SVT_OK;
            }
            if (m[j].host) {
                bcf::Sink count{nullptr, 0, 0};
                bcftext::Shape sh;
                if (bcftext::line_text(host_dict, chunk + rec_off[j], rec_off[j + 1] - rec_off[j], false, count, sh))
                    return fail(SVT_ERR_INTERNAL, "svt_bcf_text: the host refuses a record the device took");
                m[j].len = count.n;
                held.marks[from + j] = 1;
                ++info->host_lines;
            }
            text_off[j + 1] = text_off[j] + m[j].len;
        }
        const uint64_t text_bytes = text_off[k], base = held.text.size();
        if (text_bytes > text_cap) {
            if (c.d_text.p) {
                HIP_TRY(hipFree(c.d_text.p));
                c.d_text.p = nullptr;
            }
            SVT_TRY(c.d_text.alloc(text_bytes));
            text_cap = text_bytes;
        }
        SVT_TRY(h2d_staged(c.d_text_off.p, text_off.data(), (k + 1) * sizeof(uint64_t), c.s));
        SVT_TRY(c.mark(&e[3]));
        hipLaunchKernelGGL(svt_bcf_text_write_kernel, dim3(grid), dim3(kBcfTextBlock), 0, c.s, c.d_stream.as<uint8_t>(), bytes, c.d_rec_off.as<uint64_t>(), k, d,
                           c.d_measures.as<bcftext::TextMeasure>(), c.d_text_off.as<uint64_t>(), c.d_text.as<uint8_t>(), text_bytes);
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[4]));
        held.text.resize(base + text_bytes);
        SVT_TRY(d2h_staged(held.text.data() + base, c.d_text.p, text_bytes, c.s));
        SVT_TRY(c.mark(&e[5]));
        HIP_TRY(hipStreamSynchronize(c.s));
        SVT_TRY(c.between(e[3], e[4], &g_bcf_text_times.write_kernel_s));
        SVT_TRY(c.between(e[4], e[5], &g_bcf_text_times.download_s));
        for (uint64_t j = 0; j < k; ++j) {
            if (m[j].host) {
                bcf::Sink store{held.text.data() + base + text_off[j], m[j].len, 0};
                bcftext::Shape sh;
                bcftext::line_text(host_dict, chunk + rec_off[j], rec_off[j + 1] - rec_off[j], false, store, sh);
                if (store.n != store.cap) return fail(SVT_ERR_INTERNAL, "svt_bcf_text: a record's two walks disagree");
            }
            held.offsets.push_back(base + text_off[j + 1]);
        }
        from = to;
    }
    if (cut_short) {
        info->bad_record = n + 1;
        info->bad_kind = SVT_BCF_TEXT_KIND_TRUNCATED;
        held.clear();
        return SVT_OK;
    }
    info->n_records = n;
    info->text_len = held.text.size();
    info->n_offsets = held.offsets.size();
    g_bcf_text_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_bcf_text_device(const uint8_t* stream, uint64_t len, uint32_t flags, uint64_t block_bytes, svt_bcf_text_info* info, int device)
{
    return guarded([&] {
        const int rc = svt_bcf_text_device_impl(stream, len, flags, block_bytes, info, device);
        if (rc != SVT_OK) bcftext::held_result().clear();
        return rc;
    });
}

int svt_bcf_text_last_times(svt_bcf_text_times* times) { return guarded([&] { return last_times(times, g_bcf_text_times); }); }

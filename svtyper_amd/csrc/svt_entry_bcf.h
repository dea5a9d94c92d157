// svt_entry_bcf.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind svt_entry_bam_index.h;
// not a stand-alone header): VCF text as a BCF stream on the device.  What is this header's: the dictionaries' upload, the two
// launches of svt_bcf_kernel.h around the host's prefix sum (stream_resident), the records the host twin writes for the lines
// outside the float envelope, and the result left for svt_bcf_take.  What it shares lives in svt_entry_vcf_lines.h (the line
// table: lines_resident) and svt_entry_deflate.h (the upload, the members cut every dfl::kMaxPayload bytes: deflate_members).
// C ABI: svt_bcf_encode_device, svt_bcf_bgzf_device, svt_bcf_last_times (include/svtyper_bcf.h).

extern "C++" {

namespace svt {
namespace bcf {
Held& held_result();                                // (svt_reads.cpp: the calling thread's result for svt_bcf_take)
}
}

// the kernels of the calling thread's last call here, from HIP events, and the call's wall time
static thread_local svt_bcf_times g_bcf_times;

struct BcfCall : LinesCall {                                 // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_dict, d_order, d_measures, d_rec_off, d_records;
    ~BcfCall() { drain(); }
};

// the tables of `t` side by side in one allocation; the view over them
static int upload_dict(BcfCall& c, const bcf::Tables& t, bcf::Dict& d)
{
    std::vector<uint8_t> blob;
    auto add = [&](const void* p, size_t bytes) {
        const size_t at = blob.size();
        blob.insert(blob.end(), (const uint8_t*)p, (const uint8_t*)p + bytes);
        blob.resize((blob.size() + 15) & ~(size_t)15);
        return at;
    };
    const size_t name_off = add(t.name_off.data(), t.name_off.size() * 4), cname_off = add(t.cname_off.data(), t.cname_off.size() * 4);
    const size_t slots = add(t.slots.data(), t.slots.size() * 4), cslots = add(t.cslots.data(), t.cslots.size() * 4);
    const size_t names = add(t.names.data(), t.names.size()), types = add(t.types.data(), t.types.size()), cnames = add(t.cnames.data(), t.cnames.size());
    SVT_TRY(c.d_dict.alloc(blob.size()));
    SVT_TRY(h2d_staged(c.d_dict.p, blob.data(), blob.size(), c.s));
    const uint8_t* base = c.d_dict.as<uint8_t>();
    d = t.view();
    d.names = base + names;
    d.types = base + types;
    d.cnames = base + cnames;
    d.name_off = reinterpret_cast<const uint32_t*>(base + name_off);
    d.cname_off = reinterpret_cast<const uint32_t*>(base + cname_off);
    d.slots = reinterpret_cast<const int32_t*>(base + slots);
    d.cslots = reinterpret_cast<const int32_t*>(base + cslots);
    return SVT_OK;
}

// text[0, len) -> its stream in c.d_records[0, info.stream_len), offsets and spans in `held`; or info.bad_line
static int stream_resident(BcfCall& c, const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info& info, bcf::Held& held, int device)
{
    bcf::Tables t;
    if (const char* why = bcf::make_tables(text, len, t)) return fail(SVT_ERR_INVALID, std::string("svt_bcf_encode: ") + why);
    info.n_ref = (int32_t)t.n_contigs();
    info.l_ref_max = t.l_ref_max();
    info.n_sample = t.n_sample;
    SVT_TRY(c.begin(text, len));
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, text[len - 1], table, device));
    std::vector<uint64_t> order;
    if (const uint64_t bad = bcf::body_order(text, table, t, (flags & SVT_BCF_SORT) != 0, order)) {
        bcf::refuse_unsortable(t.view(), text, table, bad, info);
        return SVT_OK;
    }
    const uint64_t n = order.size();
    const bcf::Dict host_dict = t.view();
    bcf::Dict d;
    std::vector<bcf::Measure> m(n);
    // (one-wave workgroups: four where the line kernels have one of 256)
    const unsigned grid = capped_grid((n + kBcfBlock - 1) / kBcfBlock, 32, device);
    size_t e[4] = {};
    if (n) {
        SVT_TRY(upload_dict(c, t, d));
        SVT_TRY(c.d_order.alloc(n * sizeof(uint64_t)));
        SVT_TRY(h2d_staged(c.d_order.p, order.data(), n * sizeof(uint64_t), c.s));
        SVT_TRY(c.d_measures.alloc(n * sizeof(bcf::Measure)));
        SVT_TRY(c.mark(&e[0]));
        hipLaunchKernelGGL(svt_bcf_measure_kernel, dim3(grid), dim3(kBcfBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(),
                           (uint64_t)table.size(), c.d_order.as<uint64_t>(), n, d, c.d_measures.as<bcf::Measure>());
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[1]));
        SVT_TRY(d2h_staged(m.data(), c.d_measures.p, n * sizeof(bcf::Measure), c.s));
        SVT_TRY(c.between(e[0], e[1], &g_bcf_times.measure_kernel_s));
    }
    // the lines outside the envelope: the host twin's, sizes and refusals included
    for (uint64_t j = 0; j < n; ++j) {
        if (m[j].kind || !m[j].host) continue;
        bcf::Sink count{nullptr, 0, 0};
        bcf::encode_line(host_dict, text + table[order[j]].off, table[order[j]].len, false, count, m[j]);
        m[j].host = 1;
        ++info.host_lines;
    }
    std::vector<uint8_t> header;
    bcf::stream_header(text, t, header);
    info.header_len = header.size();
    if (!bcf::place_records(m, order, info.header_len, info, held)) return SVT_OK;
    info.stream_len = held.offsets[n];
    info.n_records = n;
    SVT_TRY(c.d_records.alloc(info.stream_len));
    SVT_TRY(h2d_staged(c.d_records.p, header.data(), header.size(), c.s));
    if (n) {
        SVT_TRY(c.d_rec_off.alloc((n + 1) * sizeof(uint64_t)));
        SVT_TRY(h2d_staged(c.d_rec_off.p, held.offsets.data(), (n + 1) * sizeof(uint64_t), c.s));
        SVT_TRY(c.mark(&e[2]));
        hipLaunchKernelGGL(svt_bcf_write_kernel, dim3(grid), dim3(kBcfBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(),
                           (uint64_t)table.size(), c.d_order.as<uint64_t>(), n, d, c.d_measures.as<bcf::Measure>(), c.d_rec_off.as<uint64_t>(),
                           c.d_records.as<uint8_t>(), info.stream_len);
        HIP_TRY(hipGetLastError());
        SVT_TRY(c.mark(&e[3]));
        HIP_TRY(hipStreamSynchronize(c.s));
        SVT_TRY(c.between(e[2], e[3], &g_bcf_times.write_kernel_s));
    }
    std::vector<uint8_t> record;
    for (uint64_t j = 0; j < n; ++j) {
        if (!m[j].host) continue;
        record.assign(held.offsets[j + 1] - held.offsets[j], 0);
        bcf::Sink store{record.data(), record.size(), 0};
        bcf::encode_line(host_dict, text + table[order[j]].off, table[order[j]].len, false, store, m[j]);
        if (store.n != store.cap) return fail(SVT_ERR_INTERNAL, "svt_bcf_encode: a record's two walks disagree");
        SVT_TRY(h2d_staged(c.d_records.as<uint8_t>() + held.offsets[j], record.data(), record.size(), c.s));
    }
    return SVT_OK;
}

static int bcf_check_args(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info)
{
    if (!info || !text || !len) return fail(SVT_ERR_INVALID, len || !info ? "null argument" : "svt_bcf_encode: the text has no #CHROM line");
    if (flags & ~SVT_BCF_SORT) return fail(SVT_ERR_INVALID, "svt_bcf_encode: the device routes take SVT_BCF_SORT and no other flag");
    *info = svt_bcf_info();
    g_bcf_times = svt_bcf_times();
    bcf::held_result().clear();
    return SVT_OK;
}

static int svt_bcf_encode_device_impl(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    SVT_TRY(bcf_check_args(text, len, flags, info));
    SVT_TRY(select_device(device));
    bcf::Held& held = bcf::held_result();
    BcfCall c;
    const int rc = stream_resident(c, text, len, flags, *info, held, device);
    if (rc != SVT_OK || info->bad_line) {
        held.clear();
        return rc;
    }
    held.bytes.resize(info->stream_len);
    SVT_TRY(d2h_staged(held.bytes.data(), c.d_records.p, info->stream_len, c.s));
    info->bytes_len = held.bytes.size();
    info->n_offsets = held.offsets.size();
    g_bcf_times.total_s = seconds_since(t0);
    return SVT_OK;
}

static int svt_bcf_bgzf_device_impl(const uint8_t* text, uint64_t len, uint32_t flags, uint32_t mode, svt_bcf_info* info, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_deflate_times = svt_deflate_times();
    SVT_TRY(deflate_check_mode("svt_bcf_bgzf", mode));
    SVT_TRY(bcf_check_args(text, len, flags, info));
    SVT_TRY(select_device(device));
    bcf::Held& held = bcf::held_result();
    BcfCall c;
    int rc = stream_resident(c, text, len, flags, *info, held, device);
    if (rc == SVT_OK && !info->bad_line) {
        held.starts.clear();                                    // cut where bgzf.BgzfWriter cuts
        for (uint64_t at = 0; at < info->stream_len; at += dfl::kMaxPayload) held.starts.push_back(at);
        held.starts.push_back(info->stream_len);
        const uint64_t members = held.starts.size() - 1;
        held.offsets.assign(members + 1, 0);
        held.bytes.resize(info->stream_len + members * 64);
        rc = deflate_members(c, "svt_bcf_bgzf", c.d_records.as<uint8_t>(), held.starts.data(), members, held.bytes.data(), held.bytes.size(),
                             held.offsets.data(), mode, device);
        if (rc == SVT_OK) held.bytes.resize(held.offsets[members]);
    }
    if (rc != SVT_OK || info->bad_line) {
        held.clear();
        return rc;
    }
    info->bytes_len = held.bytes.size();
    info->n_offsets = held.offsets.size();
    g_bcf_times.total_s = g_deflate_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_bcf_encode_device(const uint8_t* text, uint64_t len, uint32_t flags, svt_bcf_info* info, int device)
{
    return guarded([&] { return svt_bcf_encode_device_impl(text, len, flags, info, device); });
}

int svt_bcf_bgzf_device(const uint8_t* text, uint64_t len, uint32_t flags, uint32_t mode, svt_bcf_info* info, int device)
{
    return guarded([&] { return svt_bcf_bgzf_device_impl(text, len, flags, mode, info, device); });
}

int svt_bcf_last_times(svt_bcf_times* times) { return guarded([&] { return last_times(times, g_bcf_times); }); }

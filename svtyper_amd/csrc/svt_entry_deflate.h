// svt_entry_deflate.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// BGZF deflate on the device.  Payloads go up, svt_crc32_kernel and svt_deflate_kernel run over the same jobs on the call's
// stream, the sizes come back for a prefix sum on the host, svt_deflate_pack_kernel puts the members side by side, and they
// come down.  C ABI: svt_bgzf_deflate_device, svt_bgzf_deflate_device_mode, svt_bgzf_deflate_last_times, and the code-length rule
// on its own, svt_huffman_lengths_device (include/svtyper_reads.h).

extern "C++" {

// the three kernels of the calling thread's last svt_bgzf_deflate_device, from HIP events, and the call's wall time
static thread_local svt_deflate_times g_deflate_times;

// a device call that compresses: its stream, the buffers of the members' way through the kernels, the events around the three kernels
struct DeflateCall : CallStream {                            // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_bytes, d_jobs, d_tables, d_crc, d_clen, d_slots, d_out_off, d_out;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    ~DeflateCall()
    {
        drain();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
};

// the payloads `jobs` of d_bytes[0, payload_bytes), device memory that c.s has filled -> their members in out, out_off[0 .. n]
static int deflate_resident(DeflateCall& c, const uint8_t* d_bytes, uint64_t payload_bytes, const std::vector<crc::Job>& jobs, uint64_t slots, uint8_t* out,
                            uint64_t capacity, uint64_t* out_off, uint32_t mode, int device)
{
    const uint64_t n = jobs.size();
    for (hipEvent_t& e : c.ev) HIP_TRY(hipEventCreate(&e));
    SVT_TRY(c.d_crc.alloc(n * sizeof(uint32_t)));
    SVT_TRY(c.d_clen.alloc(n * sizeof(uint32_t)));
    SVT_TRY(c.d_slots.alloc(slots));
    SVT_TRY(c.d_out_off.alloc((n + 1) * sizeof(uint64_t)));
    {
        Stager st(c.s);
        SVT_TRY(upload(c.d_jobs, jobs, st));
        SVT_TRY(upload_crc_tables(c.d_tables, st));
        SVT_TRY(st.finish());
    }
    const uint64_t waves = (uint64_t)std::max<uint32_t>(cu_count(device), 1) * kDeflateWavesPerCu;
    HIP_TRY(hipEventRecord(c.ev[0], c.s));
    SVT_TRY(launch_crc_kernel(d_bytes, payload_bytes, c.d_jobs.as<crc::Job>(), n, c.d_tables.as<crc::Tables>(), c.d_crc.as<uint32_t>(), nullptr,
                              device, c.s));
    HIP_TRY(hipEventRecord(c.ev[1], c.s));
    hipLaunchKernelGGL(mode == SVT_DEFLATE_DYNAMIC ? svt_deflate_kernel<dfl::kDynamic> : svt_deflate_kernel<dfl::kFixed>, dim3((unsigned)std::min(n, waves)), dim3(kDeflateBlock), 0, c.s, d_bytes, payload_bytes,
                       c.d_jobs.as<crc::Job>(), (uint32_t)n, c.d_slots.as<uint8_t>(), slots, c.d_clen.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[2], c.s));
    std::vector<uint32_t> clen(n);
    HIP_TRY(hipMemcpyAsync(clen.data(), c.d_clen.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    for (uint64_t k = 0; k < n; ++k) {
        if (clen[k] == 0 || clen[k] > dfl::cdata_bound(jobs[k].len)) return fail(SVT_ERR_HIP, "svt_deflate_kernel refused a payload");
        out_off[k + 1] = out_off[k] + dfl::kHeaderBytes + clen[k] + dfl::kTrailerBytes;
    }
    if (out_off[n] > capacity) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: capacity is below what the members need");
    SVT_TRY(c.d_out.alloc(out_off[n]));
    HIP_TRY(hipMemcpyAsync(c.d_out_off.p, out_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipEventRecord(c.ev[3], c.s));
    hipLaunchKernelGGL(svt_deflate_pack_kernel, dim3((unsigned)std::min(n, waves * 4)), dim3(kDeflatePackBlock), 0, c.s, c.d_slots.as<uint8_t>(), slots,
                       c.d_jobs.as<crc::Job>(), c.d_clen.as<uint32_t>(), c.d_crc.as<uint32_t>(), c.d_out_off.as<uint64_t>(), (uint32_t)n, c.d_out.as<uint8_t>(),
                       out_off[n]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[4], c.s));
    SVT_TRY(d2h_staged(out, c.d_out.p, out_off[n], c.s));
    float crc_ms = 0, deflate_ms = 0, pack_ms = 0;
    HIP_TRY(hipEventElapsedTime(&crc_ms, c.ev[0], c.ev[1]));
    HIP_TRY(hipEventElapsedTime(&deflate_ms, c.ev[1], c.ev[2]));
    HIP_TRY(hipEventElapsedTime(&pack_ms, c.ev[3], c.ev[4]));
    g_deflate_times.crc_kernel_s = crc_ms * 1e-3;
    g_deflate_times.deflate_kernel_s = deflate_ms * 1e-3;
    g_deflate_times.pack_kernel_s = pack_ms * 1e-3;
    return SVT_OK;
}

static int svt_bgzf_deflate_device_impl(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint32_t mode,
                                        int device)
{
    if (mode != SVT_DEFLATE_FIXED && mode != SVT_DEFLATE_DYNAMIC)
        return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: mode is SVT_DEFLATE_FIXED (0) or SVT_DEFLATE_DYNAMIC (1)");
    const auto t0 = std::chrono::steady_clock::now();
    g_deflate_times = svt_deflate_times();
    uint64_t slots = 0;
    SVT_TRY(deflate_check_args(bytes, off, n, out, out_off, slots));
    SVT_TRY(select_device(device));
    out_off[0] = 0;
    if (n == 0) return SVT_OK;
    DeflateCall c;
    SVT_TRY(c.take());
    const uint64_t payload_bytes = off[n] - off[0];
    std::vector<crc::Job> jobs(n);
    for (uint64_t k = 0; k < n; ++k) jobs[k] = crc::Job{off[k] - off[0], (uint32_t)(off[k + 1] - off[k]), 0};
    SVT_TRY(c.d_bytes.alloc(payload_bytes));
    if (payload_bytes) {
        Stager st(c.s);
        SVT_TRY(st.copy(c.d_bytes.p, bytes + off[0], payload_bytes));
        SVT_TRY(st.finish());
    }
    SVT_TRY(deflate_resident(c, c.d_bytes.as<uint8_t>(), payload_bytes, jobs, slots, out, capacity, out_off, mode, device));
    g_deflate_times.total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return SVT_OK;
}

}  // extern "C++"

int svt_bgzf_deflate_device(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off, int device)
{
    return guarded([&] { return svt_bgzf_deflate_device_impl(bytes, off, n, out, capacity, out_off, SVT_DEFLATE_FIXED, device); });
}

int svt_bgzf_deflate_device_mode(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint32_t mode,
                                 int device)
{
    return guarded([&] { return svt_bgzf_deflate_device_impl(bytes, off, n, out, capacity, out_off, mode, device); });
}

int svt_huffman_lengths_device(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, uint8_t* lengths, int device)
{
    return guarded([&]() -> int {
        SVT_TRY(huffman_check_args(freq, sets, symbols, limit, lengths));
        SVT_TRY(select_device(device));
        if (sets == 0) return SVT_OK;
        struct Call : CallStream {                           // (destruction order: CallStream, svt_batch_state.h)
            DevScratch d_freq, d_len;
            ~Call() { drain(); }
        } c;
        SVT_TRY(c.take());
        const uint64_t count = (uint64_t)sets * symbols;
        SVT_TRY(c.d_freq.alloc(count * sizeof(uint32_t)));
        SVT_TRY(c.d_len.alloc(count));
        {
            Stager st(c.s);
            SVT_TRY(st.copy(c.d_freq.p, freq, count * sizeof(uint32_t)));
            SVT_TRY(st.finish());
        }
        const uint64_t waves = (uint64_t)std::max<uint32_t>(cu_count(device), 1) * kDeflateWavesPerCu;
        hipLaunchKernelGGL(svt_huffman_lengths_kernel, dim3((unsigned)std::min<uint64_t>(sets, waves)), dim3(kDeflateBlock), 0, c.s, c.d_freq.as<uint32_t>(), sets,
                           symbols, limit, c.d_len.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        SVT_TRY(d2h_staged(lengths, c.d_len.p, count, c.s));
        return SVT_OK;
    });
}

int svt_bgzf_deflate_last_times(svt_deflate_times* times)
{
    return guarded([&]() -> int {
        if (!times) return fail(SVT_ERR_INVALID, "null argument");
        *times = g_deflate_times;
        return SVT_OK;
    });
}

// svt_entry_rans.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// a batch of rANS 4x8 blocks (CRAM 3.0 block method 4) decoded on the device.  The blocks go up as they lie, the headers are
// checked on the host (svt_rans_batch.h), the order-0 and the order-1 blocks are one launch each of svt_rans_kernel.h, the output
// comes down.  The device's output buffer mirrors the caller's: where that one has bytes outside the blocks' ranges (guard
// bytes, the zeroed range of a refused header) it goes up first, so that what comes back differs from it only where a kernel
// wrote.  C ABI: svt_rans_decode_device, svt_rans_last_times (include/svtyper_reads.h).

extern "C++" {

static thread_local svt_rans_times g_rans_times;

struct RansCall : TimedCallStream {                          // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_data, d_out, d_jobs0, d_jobs1, d_status;
    ~RansCall() { drain(); }
};

static int svt_rans_decode_device_impl(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off,
                                       const uint64_t* out_size, uint8_t* out, uint64_t out_len, uint32_t* status, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_rans_times = svt_rans_times();
    std::vector<rans::Job> order0, order1;
    SVT_TRY(rans::plan_batch(data, data_len, off, n, out_off, out_size, out, out_len, status, order0, order1));
    SVT_TRY(select_device(device));
    if (order0.empty() && order1.empty()) return SVT_OK;
    uint64_t covered = 0;
    for (const auto& j : order0) covered += j.out_len;
    for (const auto& j : order1) covered += j.out_len;
    RansCall c;
    SVT_TRY(c.take());
    SVT_TRY(c.d_data.alloc(data_len));
    SVT_TRY(c.d_out.alloc(out_len));
    SVT_TRY(c.d_status.alloc(n * sizeof(uint32_t)));
    size_t e[6] = {};
    SVT_TRY(c.mark(&e[0]));
    SVT_TRY(h2d_staged(c.d_data.p, data, data_len, c.s));
    if (covered != out_len) SVT_TRY(h2d_staged(c.d_out.p, out, out_len, c.s));
    SVT_TRY(h2d_staged(c.d_status.p, status, n * sizeof(uint32_t), c.s));
    {
        Stager st(c.s);
        SVT_TRY(upload(c.d_jobs0, order0, st));
        SVT_TRY(upload(c.d_jobs1, order1, st));
        SVT_TRY(st.finish());
    }
    SVT_TRY(c.mark(&e[1]));
    if (!order0.empty()) {
        const unsigned grid = capped_grid((order0.size() + kRansQuads - 1) / kRansQuads, 16, device);
        hipLaunchKernelGGL(svt_rans_o0_kernel, dim3(grid), dim3(kRansBlock), 0, c.s, c.d_data.as<uint8_t>(), c.d_out.as<uint8_t>(), c.d_jobs0.as<rans::Job>(),
                           (uint32_t)order0.size(), c.d_status.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    SVT_TRY(c.mark(&e[2]));
    if (!order1.empty()) {
        static std::once_flag once;
        static hipError_t attr = hipSuccess;
        std::call_once(once, [] {
            attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&svt_rans_o1_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRansO1Lds);
        });
        HIP_TRY(attr);
        const unsigned grid = capped_grid(order1.size(), 1, device);       // (131 584 bytes of LDS: one workgroup per CU)
        hipLaunchKernelGGL(svt_rans_o1_kernel, dim3(grid), dim3(kRansBlock), kRansO1Lds, c.s, c.d_data.as<uint8_t>(), c.d_out.as<uint8_t>(),
                           c.d_jobs1.as<rans::Job>(), (uint32_t)order1.size(), c.d_status.as<uint32_t>());
        HIP_TRY(hipGetLastError());
    }
    SVT_TRY(c.mark(&e[3]));
    SVT_TRY(d2h_staged(out, c.d_out.p, out_len, c.s));
    SVT_TRY(d2h_staged(status, c.d_status.p, n * sizeof(uint32_t), c.s));
    SVT_TRY(c.mark(&e[4]));
    HIP_TRY(hipStreamSynchronize(c.s));
    SVT_TRY(c.between(e[0], e[1], &g_rans_times.upload_s));
    SVT_TRY(c.between(e[1], e[2], &g_rans_times.order0_kernel_s));
    SVT_TRY(c.between(e[2], e[3], &g_rans_times.order1_kernel_s));
    SVT_TRY(c.between(e[3], e[4], &g_rans_times.download_s));
    g_rans_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_rans_decode_device(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off, const uint64_t* out_size,
                           uint8_t* out, uint64_t out_len, uint32_t* status, int device)
{
    return guarded([&] { return svt_rans_decode_device_impl(data, data_len, off, n, out_off, out_size, out, out_len, status, device); });
}

int svt_rans_last_times(svt_rans_times* times) { return guarded([&] { return last_times(times, g_rans_times); }); }

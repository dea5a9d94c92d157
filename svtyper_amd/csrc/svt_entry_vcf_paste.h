// svt_entry_vcf_paste.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_vcf_lines.h; not a stand-alone header): per-sample VCFs joined by line number on the device.  What is this header's:
// the two launches of svt_vcf_paste_kernel.h around the host's plan (paste::plan_block), the marked lines written into the same
// buffer, the times.  What it shares lives in svt_entry_vcf_lines.h (the line table: lines_resident) and svt_entry_deflate.h (the
// upload: OrderedCall::begin).  C ABI: svt_vcf_paste_device, svt_vcf_paste_last_times (include/svtyper_reads.h).

extern "C++" {

// the kernels of the calling thread's last call here, from HIP events; its copies and the call on the host's clock
static thread_local svt_vcf_paste_times g_paste_times;

// How the write kernel spreads its lanes over the sample parts where the caller does not say: a quarter of the wavefront per
// part (DESIGN 3.4 has the measurement)
constexpr uint32_t kPasteLayout = 2;

struct PasteCall : LinesCall {                               // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_first, d_results, d_places, d_prefixes, d_prefix_off, d_out_off, d_out;
    ~PasteCall() { drain(); }
};

static int svt_vcf_paste_device_impl(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines, uint32_t flags,
                                     const uint8_t* info_table, uint64_t info_len, uint8_t* out, uint64_t capacity, svt_paste_line* results,
                                     svt_paste_info* info, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_paste_times = svt_vcf_paste_times();
    g_lines_times = svt_vcf_lines_times();
    paste::Block b;
    if (const char* why = paste::take_arguments(text, len, first_line, n_inputs, n_lines, flags, info_table, info_len, out, results, info, b))
        return fail(SVT_ERR_INVALID, why);
    if (!n_inputs) return fail(SVT_ERR_INVALID, "svt_vcf_paste: no input");
    SVT_TRY(select_device(device));
    if (!n_lines || !len) return SVT_OK;
    uint32_t layout = flags >> SVT_PASTE_LAYOUT_SHIFT & 3u;
    if (!layout) layout = kPasteLayout;
    PasteCall c;
    auto t = std::chrono::steady_clock::now();
    SVT_TRY(c.begin(text, len));
    HIP_TRY(hipStreamSynchronize(c.s));
    g_paste_times.upload_s = seconds_since(t);
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, text[len - 1], table, device));
    g_paste_times.lines_kernels_s = lines_kernels_s();
    b.lines = table.data();
    b.n_table = table.size();
    if (const char* why = paste::check_block(b)) return fail(SVT_ERR_INVALID, why);
    const uint64_t cells = n_lines * n_inputs;
    SVT_TRY(c.d_first.alloc(((uint64_t)n_inputs + 1) * sizeof(uint64_t)));
    SVT_TRY(h2d_staged(c.d_first.p, first_line, ((uint64_t)n_inputs + 1) * sizeof(uint64_t), c.s));
    SVT_TRY(c.d_results.alloc(n_lines * sizeof(svt_paste_line)));
    SVT_TRY(c.d_places.alloc(cells * sizeof(paste::Place)));
    const unsigned grid = capped_grid((n_lines + kPasteWaves - 1) / kPasteWaves, 16, device);
    size_t e[4] = {};
    SVT_TRY(c.mark(&e[0]));
    hipLaunchKernelGGL(svt_paste_measure_kernel, dim3(grid), dim3(kPasteBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(),
                       (uint64_t)table.size(), c.d_first.as<uint64_t>(), n_inputs, n_lines, b.flags, c.d_results.as<svt_paste_line>(),
                       c.d_places.as<paste::Place>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(results, c.d_results.p, n_lines * sizeof(svt_paste_line), c.s));
    g_paste_times.download_s += seconds_since(t);
    SVT_TRY(c.between(e[0], e[1], &g_paste_times.measure_kernel_s));
    // the host step: the marked lines, the other lines' first columns, where every line goes
    t = std::chrono::steady_clock::now();
    paste::Plan plan;
    paste::Bad bad;
    if (const uint64_t bad_line = paste::plan_block(b, results, plan, bad)) {
        paste::report(*info, bad_line, bad);
        return SVT_OK;
    }
    g_paste_times.host_s = seconds_since(t);
    info->host_lines = plan.host_lines;
    info->out_len = plan.out_off[n_lines];
    if (info->out_len > capacity) return fail(SVT_ERR_INVALID, "svt_vcf_paste: capacity is below the pasted text");
    // (the plan changed flags and line_len of the marked lines: the write kernel reads the results for the marks and part_len)
    SVT_TRY(h2d_staged(c.d_results.p, results, n_lines * sizeof(svt_paste_line), c.s));
    SVT_TRY(c.d_prefixes.alloc(plan.prefixes.size()));
    if (!plan.prefixes.empty()) SVT_TRY(h2d_staged(c.d_prefixes.p, plan.prefixes.data(), plan.prefixes.size(), c.s));
    SVT_TRY(c.d_prefix_off.alloc((n_lines + 1) * sizeof(uint64_t)));
    SVT_TRY(h2d_staged(c.d_prefix_off.p, plan.prefix_off.data(), (n_lines + 1) * sizeof(uint64_t), c.s));
    SVT_TRY(c.d_out_off.alloc((n_lines + 1) * sizeof(uint64_t)));
    SVT_TRY(h2d_staged(c.d_out_off.p, plan.out_off.data(), (n_lines + 1) * sizeof(uint64_t), c.s));
    SVT_TRY(c.d_out.alloc(info->out_len));
    SVT_TRY(c.mark(&e[2]));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kPasteBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), (uint64_t)table.size(),
                           c.d_first.as<uint64_t>(), n_inputs, n_lines, c.d_results.as<svt_paste_line>(), c.d_places.as<paste::Place>(),
                           c.d_prefixes.as<uint8_t>(), (uint64_t)plan.prefixes.size(), c.d_prefix_off.as<uint64_t>(), c.d_out_off.as<uint64_t>(),
                           c.d_out.as<uint8_t>(), info->out_len);
    };
    if (layout == 1) launch(svt_paste_write_kernel<1>);
    else if (layout == 2) launch(svt_paste_write_kernel<16>);
    else launch(svt_paste_write_kernel<64>);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[3]));
    for (const auto& l : plan.slow)                             // the host twin's lines, into the same buffer
        SVT_TRY(h2d_staged(c.d_out.as<uint8_t>() + plan.out_off[l.first], l.second.data(), l.second.size(), c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    t = std::chrono::steady_clock::now();
    SVT_TRY(d2h_staged(out, c.d_out.p, info->out_len, c.s));
    g_paste_times.download_s += seconds_since(t);
    SVT_TRY(c.between(e[2], e[3], &g_paste_times.write_kernel_s));
    g_paste_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_vcf_paste_device(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines, uint32_t flags,
                         const uint8_t* info_table, uint64_t info_len, uint8_t* out, uint64_t capacity, svt_paste_line* results, svt_paste_info* info,
                         int device)
{
    return guarded([&] {
        return svt_vcf_paste_device_impl(text, len, first_line, n_inputs, n_lines, flags, info_table, info_len, out, capacity, results, info, device);
    });
}

int svt_vcf_paste_last_times(svt_vcf_paste_times* times) { return guarded([&] { return last_times(times, g_paste_times); }); }

// svt_entry_vcf_lines.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_deflate.h; not a stand-alone header): VCF text as lines on the device.  What is this header's: the line table
// (lines_resident: svt_vcf_count_kernel counts newlines per tile, the counts come down for a prefix sum on the host,
// svt_vcf_starts_kernel and svt_vcf_parse_kernel write the table), the argument checks and the caller's arrays.  What it shares
// lives in svt_entry_deflate.h: the upload (OrderedCall::begin), the gather (gather_resident<svt_tbx_line>), the members cut every
// dfl::kMaxPayload bytes (deflate_members), the marks that time the kernels.  C ABI: svt_vcf_lines_device, svt_vcf_gather_device,
// svt_vcf_bgzf_device (table, order, gather and the deflate kernels over one upload), svt_vcf_lines_last_times
// (include/svtyper_reads.h).

extern "C++" {

// the kernels of the calling thread's last call here, from HIP events, and the call's wall time
static thread_local svt_vcf_lines_times g_lines_times;

// what lines_resident's three kernels took together: the lines_kernels_s of the calls that make their line table with it
static double lines_kernels_s() { return g_lines_times.count_kernel_s + g_lines_times.starts_kernel_s + g_lines_times.parse_kernel_s; }

struct LinesCall : OrderedCall {                             // (svt_entry_deflate.h; destruction order: CallStream, svt_batch_state.h)
    DevScratch d_counts, d_base, d_lines;
    ~LinesCall() { drain(); }
};

// c.d_stream[0, len) -> its line table in c.d_lines and in `table`; `last` is the text's last byte
static int lines_resident(LinesCall& c, uint64_t len, uint8_t last, std::vector<svt_tbx_line>& table, int device)
{
    table.clear();
    if (len == 0) return SVT_OK;
    const uint64_t n_tiles = (len + tbx::kTile - 1) / tbx::kTile;
    const unsigned grid = lines_grid((n_tiles + kLinesWaves - 1) / kLinesWaves, device);
    SVT_TRY(c.d_counts.alloc(n_tiles * sizeof(uint32_t)));
    size_t e[5] = {};
    SVT_TRY(c.mark(&e[0]));
    hipLaunchKernelGGL(svt_vcf_count_kernel, dim3(grid), dim3(kLinesBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, n_tiles, c.d_counts.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    std::vector<uint32_t> counts(n_tiles);
    SVT_TRY(d2h_staged(counts.data(), c.d_counts.p, n_tiles * sizeof(uint32_t), c.s));
    std::vector<uint64_t> base(n_tiles);
    uint64_t newlines = 0;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        if (counts[t] > tbx::kTile) return fail(SVT_ERR_HIP, "svt_vcf_count_kernel counted more newlines than a tile has bytes");
        base[t] = newlines;
        newlines += counts[t];
    }
    const uint64_t n_lines = newlines + (last != '\n');
    SVT_TRY(c.d_lines.alloc(n_lines * sizeof(svt_tbx_line)));
    HIP_TRY(hipMemsetAsync(c.d_lines.p, 0, n_lines * sizeof(svt_tbx_line), c.s));
    {
        Stager st(c.s);
        SVT_TRY(upload(c.d_base, base, st));
        SVT_TRY(st.finish());
    }
    SVT_TRY(c.mark(&e[2]));
    hipLaunchKernelGGL(svt_vcf_starts_kernel, dim3(grid), dim3(kLinesBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, n_tiles, c.d_base.as<uint64_t>(),
                       c.d_lines.as<svt_tbx_line>(), n_lines);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[3]));
    hipLaunchKernelGGL(svt_vcf_parse_kernel, dim3(lines_grid((n_lines + kLinesBlock - 1) / kLinesBlock, device)), dim3(kLinesBlock), 0, c.s,
                       c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n_lines);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[4]));
    table.resize(n_lines);
    SVT_TRY(d2h_staged(table.data(), c.d_lines.p, n_lines * sizeof(svt_tbx_line), c.s));
    SVT_TRY(c.between(e[0], e[1], &g_lines_times.count_kernel_s));
    SVT_TRY(c.between(e[2], e[3], &g_lines_times.starts_kernel_s));
    SVT_TRY(c.between(e[3], e[4], &g_lines_times.parse_kernel_s));
    // the kernels' table tiles the text or it is not theirs: what the gather and the callers rely on
    uint64_t at = 0;
    for (const svt_tbx_line& l : table) {
        if (l.off != at || l.len > len - at) return fail(SVT_ERR_HIP, "svt_vcf_starts_kernel: the lines do not tile the text");
        at += l.len;
    }
    if (at != len) return fail(SVT_ERR_HIP, "svt_vcf_starts_kernel: the lines do not tile the text");
    return SVT_OK;
}

static int svt_vcf_lines_device_impl(const uint8_t* text, uint64_t len, svt_tbx_line* lines, uint64_t capacity, uint64_t* n_lines, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_lines_times = svt_vcf_lines_times();
    if (!n_lines || (len && !text)) return fail(SVT_ERR_INVALID, "null argument");
    *n_lines = 0;
    SVT_TRY(select_device(device));
    LinesCall c;
    SVT_TRY(c.begin(text, len));
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, len ? text[len - 1] : (uint8_t)'\n', table, device));
    *n_lines = table.size();
    if (table.size() > capacity) return fail(SVT_ERR_INVALID, "svt_vcf_lines: capacity is below the number of lines");
    if (!table.empty() && !lines) return fail(SVT_ERR_INVALID, "null argument");
    if (!table.empty()) std::memcpy(lines, table.data(), table.size() * sizeof(svt_tbx_line));
    g_lines_times.total_s = seconds_since(t0);
    return SVT_OK;
}

static int svt_vcf_gather_device_impl(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm, uint64_t n_perm,
                                      uint8_t* out, uint64_t out_len, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_lines_times = svt_vcf_lines_times();
    if ((len && !text) || (n && !lines) || (n_perm && !perm) || (out_len && !out)) return fail(SVT_ERR_INVALID, "null argument");
    std::vector<uint64_t> dst_off;
    if (const char* why = tbx::gather_plan(len, lines, n, perm, n_perm, out_len, dst_off)) return fail(SVT_ERR_INVALID, why);
    SVT_TRY(select_device(device));
    LinesCall c;
    SVT_TRY(c.begin(text, len));
    SVT_TRY(c.d_lines.alloc(n * sizeof(svt_tbx_line)));
    if (n) SVT_TRY(h2d_staged(c.d_lines.p, lines, n * sizeof(svt_tbx_line), c.s));
    SVT_TRY(c.d_sorted.alloc(out_len));
    SVT_TRY(gather_resident(c, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n, perm, dst_off, c.d_sorted.as<uint8_t>(), out_len,
                            &g_lines_times.gather_kernel_s, device));
    if (out_len) SVT_TRY(d2h_staged(out, c.d_sorted.p, out_len, c.s));
    g_lines_times.total_s = seconds_since(t0);
    return SVT_OK;
}

static int svt_vcf_bgzf_device_impl(const uint8_t* text, uint64_t len, int sort, uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off,
                                    svt_tbx_line* lines, uint64_t line_capacity, uint64_t* n_lines, uint64_t* src_off, uint64_t* bad_line, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_lines_times = svt_vcf_lines_times();
    g_deflate_times = svt_deflate_times();
    SVT_TRY(deflate_check_mode("svt_vcf_bgzf", mode));
    if (!out_off || !n_lines || !bad_line || (len && (!text || !out))) return fail(SVT_ERR_INVALID, "null argument");
    *n_lines = 0;
    *bad_line = 0;
    out_off[0] = 0;
    SVT_TRY(select_device(device));
    if (len == 0) return SVT_OK;
    LinesCall c;
    SVT_TRY(c.begin(text, len));
    std::vector<svt_tbx_line> table;
    SVT_TRY(lines_resident(c, len, text[len - 1], table, device));
    const uint64_t n = table.size();
    *n_lines = n;
    if (n > line_capacity) return fail(SVT_ERR_INVALID, "svt_vcf_bgzf: line_capacity is below the number of lines");
    if (!lines || !src_off) return fail(SVT_ERR_INVALID, "null argument");
    const uint8_t* d_written = c.d_stream.as<uint8_t>();
    if (sort) {
        std::vector<uint64_t> perm(n), dst_off;
        *bad_line = tbx::sort_order(text, table.data(), n, perm.data());
        if (*bad_line) return SVT_OK;
        if (const char* why = tbx::gather_plan(len, table.data(), n, perm.data(), n, len, dst_off)) return fail(SVT_ERR_INTERNAL, why);
        SVT_TRY(c.d_sorted.alloc(len));
        SVT_TRY(gather_resident(c, c.d_stream.as<uint8_t>(), len, c.d_lines.as<svt_tbx_line>(), n, perm.data(), dst_off, c.d_sorted.as<uint8_t>(), len,
                                &g_lines_times.gather_kernel_s, device));
        d_written = c.d_sorted.as<uint8_t>();
        for (uint64_t j = 0; j < n; ++j) {
            lines[j] = table[perm[j]];
            src_off[j] = lines[j].off;
            lines[j].off = dst_off[j];
        }
    } else {
        for (uint64_t j = 0; j < n; ++j) {
            lines[j] = table[j];
            src_off[j] = table[j].off;
        }
    }
    std::vector<uint64_t> start;                                // cut where bgzf.BgzfWriter cuts
    for (uint64_t at = 0; at < len; at += dfl::kMaxPayload) start.push_back(at);
    start.push_back(len);
    SVT_TRY(deflate_members(c, "svt_vcf_bgzf", d_written, start.data(), start.size() - 1, out, capacity, out_off, mode, device));
    g_lines_times.total_s = g_deflate_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_vcf_lines_device(const uint8_t* text, uint64_t len, svt_tbx_line* lines, uint64_t capacity, uint64_t* n_lines, int device)
{
    return guarded([&] { return svt_vcf_lines_device_impl(text, len, lines, capacity, n_lines, device); });
}

int svt_vcf_gather_device(const uint8_t* text, uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm, uint64_t n_perm, uint8_t* out,
                          uint64_t out_len, int device)
{
    return guarded([&] { return svt_vcf_gather_device_impl(text, len, lines, n, perm, n_perm, out, out_len, device); });
}

int svt_vcf_bgzf_device(const uint8_t* text, uint64_t len, int sort, uint32_t mode, uint8_t* out, uint64_t capacity, uint64_t* out_off, svt_tbx_line* lines,
                        uint64_t line_capacity, uint64_t* n_lines, uint64_t* src_off, uint64_t* bad_line, int device)
{
    return guarded([&] {
        return svt_vcf_bgzf_device_impl(text, len, sort, mode, out, capacity, out_off, lines, line_capacity, n_lines, src_off, bad_line, device);
    });
}

int svt_vcf_lines_last_times(svt_vcf_lines_times* times) { return guarded([&] { return last_times(times, g_lines_times); }); }

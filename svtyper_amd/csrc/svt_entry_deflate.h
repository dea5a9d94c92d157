// svt_entry_deflate.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// BGZF deflate on the device.  Payloads go up, svt_crc32_kernel and svt_deflate_kernel run over the same jobs on the call's
// stream, the sizes come back for a prefix sum on the host, svt_deflate_pack_kernel puts the members side by side, and they
// come down (deflate_resident).  What the entries that hold a whole output share with this one also lives here, once:
// deflate_check_mode, deflate_members (member boundaries -> crc::Jobs and slots -> deflate_resident), OrderedCall (the uploaded
// stream, its order, the gathered stream) and gather_resident<Row> (the gather kernel over a line or a span table); the kernels'
// times are marks on the call's stream (TimedCallStream, svt_batch_state.h).  C ABI: svt_bgzf_deflate_device,
// svt_bgzf_deflate_device_mode, svt_bgzf_deflate_last_times, svt_huffman_lengths_device (include/svtyper_reads.h).

extern "C++" {

// the three kernels of the calling thread's last svt_bgzf_deflate_device, from HIP events, and the call's wall time
static thread_local svt_deflate_times g_deflate_times;

// the body of svt_bgzf_deflate_last_times, svt_vcf_lines_last_times and svt_bam_sort_last_times
template <typename Times>
static int last_times(Times* times, const Times& last)
{
    if (!times) return fail(SVT_ERR_INVALID, "null argument");
    *times = last;
    return SVT_OK;
}

// a device call that compresses: its stream with the marks around its kernels, the buffers of the members' way through the kernels
struct DeflateCall : TimedCallStream {                       // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_bytes, d_jobs, d_tables, d_crc, d_clen, d_slots, d_out_off, d_out;
    ~DeflateCall() { drain(); }
};

// the payloads `jobs` of d_bytes[0, payload_bytes), device memory that c.s has filled -> their members in out, out_off[0 .. n]
static int deflate_resident(DeflateCall& c, const uint8_t* d_bytes, uint64_t payload_bytes, const std::vector<crc::Job>& jobs, uint64_t slots, uint8_t* out,
                            uint64_t capacity, uint64_t* out_off, uint32_t mode, int device)
{
    const uint64_t n = jobs.size();
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
    size_t e[5] = {};
    SVT_TRY(c.mark(&e[0]));
    SVT_TRY(launch_crc_kernel(d_bytes, payload_bytes, c.d_jobs.as<crc::Job>(), n, c.d_tables.as<crc::Tables>(), c.d_crc.as<uint32_t>(), nullptr,
                              device, c.s));
    SVT_TRY(c.mark(&e[1]));
    hipLaunchKernelGGL(mode == SVT_DEFLATE_DYNAMIC ? svt_deflate_kernel<dfl::kDynamic> : svt_deflate_kernel<dfl::kFixed>, dim3((unsigned)std::min(n, waves)), dim3(kDeflateBlock), 0, c.s, d_bytes, payload_bytes,
                       c.d_jobs.as<crc::Job>(), (uint32_t)n, c.d_slots.as<uint8_t>(), slots, c.d_clen.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[2]));
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
    SVT_TRY(c.mark(&e[3]));
    hipLaunchKernelGGL(svt_deflate_pack_kernel, dim3((unsigned)std::min(n, waves * 4)), dim3(kDeflatePackBlock), 0, c.s, c.d_slots.as<uint8_t>(), slots,
                       c.d_jobs.as<crc::Job>(), c.d_clen.as<uint32_t>(), c.d_crc.as<uint32_t>(), c.d_out_off.as<uint64_t>(), (uint32_t)n, c.d_out.as<uint8_t>(),
                       out_off[n]);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[4]));
    SVT_TRY(d2h_staged(out, c.d_out.p, out_off[n], c.s));
    SVT_TRY(c.between(e[0], e[1], &g_deflate_times.crc_kernel_s));
    SVT_TRY(c.between(e[1], e[2], &g_deflate_times.deflate_kernel_s));
    SVT_TRY(c.between(e[3], e[4], &g_deflate_times.pack_kernel_s));
    return SVT_OK;
}

// what every entry that compresses asks of `mode`, in that entry's name
static int deflate_check_mode(const char* entry, uint32_t mode)
{
    if (mode != SVT_DEFLATE_FIXED && mode != SVT_DEFLATE_DYNAMIC)
        return fail(SVT_ERR_INVALID, std::string(entry) + ": mode is SVT_DEFLATE_FIXED (0) or SVT_DEFLATE_DYNAMIC (1)");
    return SVT_OK;
}

// From member boundaries to members: d_written holds the bytes [start[0], start[n]) of a stream, device memory that c.s has filled;
// member k is its bytes [start[k], start[k + 1]), at most dfl::kMaxPayload of them -> the members in out, out_off[0 .. n]
static int deflate_members(DeflateCall& c, const char* entry, const uint8_t* d_written, const uint64_t* start, uint64_t n, uint8_t* out, uint64_t capacity,
                           uint64_t* out_off, uint32_t mode, int device)
{
    if (n > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, std::string(entry) + ": too many members in one call (< 2^32)");
    std::vector<crc::Job> jobs(n);
    uint64_t slots = 0;
    for (uint64_t k = 0; k < n; ++k) {
        jobs[k] = crc::Job{start[k] - start[0], (uint32_t)(start[k + 1] - start[k]), 0};
        slots += dfl::slot_bytes(jobs[k].len);
    }
    return deflate_resident(c, d_written, start[n] - start[0], jobs, slots, out, capacity, out_off, mode, device);
}

// A stream that is ordered and then compressed: the uploaded stream, the order it is gathered in, the gathered stream.  Base of
// LinesCall (svt_entry_vcf_lines.h: VCF lines) and BamSortCall (svt_entry_bam_sort.h: BAM records), which add their tables.
struct OrderedCall : DeflateCall {                           // (destruction order: CallStream, svt_batch_state.h)
    DevScratch d_stream, d_perm, d_dst_off, d_sorted;
    ~OrderedCall() { drain(); }
    int begin(const uint8_t* bytes, uint64_t len)
    {
        SVT_TRY(take());
        SVT_TRY(d_stream.alloc(len));
        return h2d_staged(d_stream.p, bytes, len, s);
    }
};

// a grid of `work` workgroups, at most `per_cu` for each of the device's compute units and at least one
static unsigned capped_grid(uint64_t work, uint32_t per_cu, int device)
{
    const uint64_t most = (uint64_t)std::max<uint32_t>(cu_count(device), 1) * per_cu;
    return (unsigned)std::max<uint64_t>(std::min(work, most), 1);
}

static unsigned lines_grid(uint64_t work_groups, int device) { return capped_grid(work_groups, 8, device); }

// the rows perm[0 .. dst_off.size()) of d_src[0, len) (table d_table, n rows) side by side in d_dst[0, out_len), row perm[j] at
// dst_off[j]; the kernel's seconds are added to *kernel_s.  d_src, d_table and d_dst are device memory that c.s has filled
template <typename Row>
static int gather_resident(OrderedCall& c, const uint8_t* d_src, uint64_t len, const Row* d_table, uint64_t n, const uint64_t* perm,
                           const std::vector<uint64_t>& dst_off, uint8_t* d_dst, uint64_t out_len, double* kernel_s, int device)
{
    const uint64_t n_perm = dst_off.size();
    if (n_perm == 0) return SVT_OK;
    SVT_TRY(c.d_perm.alloc(n_perm * sizeof(uint64_t)));
    {
        Stager st(c.s);
        SVT_TRY(st.copy(c.d_perm.p, perm, n_perm * sizeof(uint64_t)));
        SVT_TRY(upload(c.d_dst_off, dst_off, st));
        SVT_TRY(st.finish());
    }
    size_t e0 = 0, e1 = 0;
    SVT_TRY(c.mark(&e0));
    hipLaunchKernelGGL(svt_vcf_gather_kernel<Row>, dim3(lines_grid(((n_perm + 63) / 64 + kLinesWaves - 1) / kLinesWaves, device)), dim3(kLinesBlock), 0, c.s, d_src,
                       len, d_table, n, c.d_perm.as<uint64_t>(), c.d_dst_off.as<uint64_t>(), n_perm, d_dst, out_len);
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e1));
    HIP_TRY(hipStreamSynchronize(c.s));
    return c.between(e0, e1, kernel_s);
}

static int svt_bgzf_deflate_device_impl(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* out, uint64_t capacity, uint64_t* out_off, uint32_t mode,
                                        int device)
{
    SVT_TRY(deflate_check_mode("svt_bgzf_deflate", mode));
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
    SVT_TRY(c.d_bytes.alloc(payload_bytes));
    if (payload_bytes) SVT_TRY(h2d_staged(c.d_bytes.p, bytes + off[0], payload_bytes, c.s));
    SVT_TRY(deflate_members(c, "svt_bgzf_deflate", c.d_bytes.as<uint8_t>(), off, n, out, capacity, out_off, mode, device));
    g_deflate_times.total_s = seconds_since(t0);
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

int svt_bgzf_deflate_last_times(svt_deflate_times* times) { return guarded([&] { return last_times(times, g_deflate_times); }); }

// svt_entry_inflate.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// the device side of a bgzf::MemberSet (svt_bgzf.h), once, for the device reader (svt_entry_evidence.h), the library scan
// (svt_entry_library.h) and the parity entries: the launchers of svt_inflate_kernel and svt_crc32_kernel and the two steps
// every caller takes around them.  C ABI: svt_bgzf_inflate_device, svt_bgzf_inflate_device_verified, svt_bgzf_crc32_device
// (include/svtyper_reads.h).

extern "C++" {

// a device buffer that is kept from call to call of its owner (the scan: from round to round) and grows when more is needed
struct GrowBuffer {
    DevScratch d;
    size_t cap = 0;
    int need(size_t bytes)
    {
        if (bytes <= cap && d.p) return SVT_OK;
        if (d.p) { HIP_TRY(hipFree(d.p)); d.p = nullptr; cap = 0; }
        const size_t want = bytes + bytes / 8 + 64;
        SVT_TRY(d.alloc(want));
        cap = want;
        return SVT_OK;
    }
    template <typename T> T* as() const { return d.as<T>(); }
};

// svt_crc32_kernel over `n` jobs on `bytes`: a grid sized to the device (its waves stage the tables once and loop over the jobs)
static int launch_crc_kernel(const uint8_t* d_bytes, uint64_t bytes_len, const crc::Job* d_jobs, uint64_t n, const crc::Tables* d_tables,
                             uint32_t* d_crc, uint32_t* d_status, int device, hipStream_t s)
{
    if (!n) return SVT_OK;
    const uint64_t waves = (uint64_t)std::max<uint32_t>(cu_count(device), 1) * kCrcWavesPerCu;
    hipLaunchKernelGGL(svt_crc32_kernel, dim3((unsigned)std::min(n, waves)), dim3(kCrcBlock), 0, s, d_bytes, bytes_len, d_jobs, (uint32_t)n, d_tables, d_crc,
                       d_status);
    HIP_TRY(hipGetLastError());
    return SVT_OK;
}

// the tables of svt_crc32.h into HBM (the buffer lives as long as `d_tables`)
static int upload_crc_tables(DevScratch& d_tables, Stager& st)
{
    SVT_TRY(d_tables.alloc(sizeof(crc::Tables)));
    return st.copy(d_tables.p, &crc_tables(), sizeof(crc::Tables));
}

// What verify adds to an inflate launch: the jobs (a member's place in the arena and the CRC-32 its trailer stores) and the
// tables in HBM, and where the figures go.  Null jobs: no verify, nothing is launched.
struct CrcCheck {
    const crc::Job* d_jobs = nullptr;
    const crc::Tables* d_tables = nullptr;
    int device = 0;
    VerifyTally* tally = nullptr;
};

// `n` members of the compressed bytes at d_src into d_dst, one wavefront each; the statuses come back in `status`.  With a
// check svt_crc32_kernel runs behind it over the same statuses (inf::INF_CRC), in a launch of its own that is timed apart.
static int run_inflate_kernel(const uint8_t* d_src, uint64_t src_len, const inf::Member* d_members, uint64_t n, uint8_t* d_dst, uint64_t dst_len,
                              uint32_t* d_status, std::vector<uint32_t>& status, hipStream_t s, const CrcCheck& check)
{
    status.assign(n, 0);
    if (n > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "too many BGZF members in one call (< 2^32)");
    constexpr uint64_t kGrid = 1u << 30;
    for (uint64_t at = 0; at < n; at += kGrid) {
        const uint64_t m = std::min(kGrid, n - at);
        hipLaunchKernelGGL(svt_inflate_kernel, dim3((unsigned)m), dim3(kInflateBlock), 0, s, d_src, src_len, d_members + at, (uint32_t)m, d_dst, dst_len,
                           d_status + at);
        HIP_TRY(hipGetLastError());
    }
    std::chrono::steady_clock::time_point t_crc;
    if (check.d_jobs && n) {
        HIP_TRY(hipStreamSynchronize(s));                        // (only so that the CRC's time is its own)
        t_crc = std::chrono::steady_clock::now();
        SVT_TRY(launch_crc_kernel(d_dst, dst_len, check.d_jobs, n, check.d_tables, nullptr, d_status, check.device, s));
    }
    if (n) HIP_TRY(hipMemcpyAsync(status.data(), d_status, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (check.d_jobs && n && check.tally) {
        uint64_t verified = 0, failed = 0;                       // (a member that did not inflate was not looked at)
        for (uint32_t st : status) { verified += st == inf::INF_OK || st == inf::INF_CRC; failed += st == inf::INF_CRC; }
        check.tally->add(verified, failed, 0.0, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_crc).count());
    }
    return SVT_OK;
}

// A MemberSet inflated on the device, in the two steps its callers time apart.  The compressed bytes and the arena are the
// caller's (a pool, buffers kept from round to round, plain scratch); here are only the small buffers, kept and grown from one
// upload() to the next (the scan's rounds), the tables going up once.  A member of the struct that holds the call's buffers.
struct DeviceInflate {
    const int device;
    GrowBuffer d_members, d_status, d_jobs;
    DevScratch d_tables;
    CrcCheck check;
    uint64_t n = 0, compressed_bytes = 0, arena_bytes = 0;
    explicit DeviceInflate(int device_) : device(device_) {}
    // the set's spans side by side into d_compressed, its member table, with `verify` the expected CRC-32s; `st` is the caller's to finish
    int upload(const bgzf::MemberSet& set, void* d_compressed, Stager& st, VerifyTally* verify)
    {
        n = set.members.size(); compressed_bytes = set.compressed_bytes; arena_bytes = set.arena_bytes;
        SVT_TRY(d_members.need(n * sizeof(inf::Member)));
        SVT_TRY(d_status.need(n * sizeof(uint32_t)));
        for (const auto& sp : set.spans) SVT_TRY(st.copy(static_cast<uint8_t*>(d_compressed) + sp.at, set.file + sp.file_off, sp.bytes));
        SVT_TRY(st.copy(d_members.d.p, set.members.data(), n * sizeof(inf::Member)));
        check = CrcCheck();
        if (verify) {
            std::vector<crc::Job> jobs;
            set.crc_jobs(jobs);
            SVT_TRY(d_jobs.need(n * sizeof(crc::Job)));
            SVT_TRY(st.copy(d_jobs.d.p, jobs.data(), n * sizeof(crc::Job)));
            if (!d_tables.p) SVT_TRY(upload_crc_tables(d_tables, st));
            check = CrcCheck{d_jobs.as<crc::Job>(), d_tables.as<crc::Tables>(), device, verify};
        }
        return SVT_OK;
    }
    // svt_inflate_kernel over what upload() left, into d_arena (arena_bytes of it), and svt_crc32_kernel behind it with verify
    int run(const void* d_compressed, void* d_arena, hipStream_t s, std::vector<uint32_t>& status)
    {
        return run_inflate_kernel(static_cast<const uint8_t*>(d_compressed), compressed_bytes, d_members.as<inf::Member>(), n, static_cast<uint8_t*>(d_arena),
                                  arena_bytes, d_status.as<uint32_t>(), status, s, check);
    }
};

}  // extern "C++"

// the parity entry of the inflate kernel: upload, one wavefront per member, download
static int svt_bgzf_inflate_device_impl(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                        const uint64_t* out_off, uint32_t* status, int device, bool verify)
{
    bgzf::MemberSet set;
    SVT_TRY(bgzf::bgzf_members(data, len, block_off, n, out, out_off, status, set));
    SVT_TRY(select_device(device));
    if (n == 0) return SVT_OK;
    struct InflateCall : CallStream {                        // (destruction order: CallStream, svt_batch_state.h)
        DevScratch d_src, d_dst;
        DeviceInflate inflate;
        explicit InflateCall(int device_) : inflate(device_) {}
        ~InflateCall() { drain(); }
    } c(device);
    SVT_TRY(c.take());
    SVT_TRY(c.d_src.alloc(len));
    SVT_TRY(c.d_dst.alloc(set.arena_bytes));
    VerifyTally uncounted;                                   // (no handle here: verify is on, nothing is reported)
    {
        Stager st(c.s);
        SVT_TRY(c.inflate.upload(set, c.d_src.p, st, verify ? &uncounted : nullptr));
        SVT_TRY(st.finish());
    }
    std::vector<uint32_t> st_host;
    SVT_TRY(c.inflate.run(c.d_src.p, c.d_dst.p, c.s, st_host));
    std::memcpy(status, st_host.data(), n * sizeof(uint32_t));
    if (set.arena_bytes) SVT_TRY(d2h_staged(out, c.d_dst.p, set.arena_bytes, c.s));
    return SVT_OK;
}

int svt_bgzf_inflate_device(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out, const uint64_t* out_off,
                            uint32_t* status, int device)
{
    return guarded([&] { return svt_bgzf_inflate_device_impl(data, len, block_off, n, out, out_off, status, device, false); });
}

int svt_bgzf_inflate_device_verified(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, uint8_t* out,
                                     const uint64_t* out_off, uint32_t* status, int device)
{
    return guarded([&] { return svt_bgzf_inflate_device_impl(data, len, block_off, n, out, out_off, status, device, true); });
}

// svt_crc32_kernel over bytes that are in HBM already: the jobs and the tables go up, the CRCs come back
int svt_bgzf_crc32_device(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t* crc, int device)
{
    return guarded([&]() -> int {
        SVT_TRY(crc_check_offsets(bytes, off, n, crc));
        SVT_TRY(select_device(device));
        if (n == 0) return SVT_OK;
        struct CrcCall : CallStream {                            // (destruction order: CallStream, svt_batch_state.h)
            DevScratch d_jobs, d_tables, d_crc;
            ~CrcCall() { drain(); }
        } c;
        SVT_TRY(c.take());
        std::vector<crc::Job> jobs(n);
        for (uint64_t k = 0; k < n; ++k) jobs[k] = crc::Job{off[k], (uint32_t)(off[k + 1] - off[k]), 0};
        SVT_TRY(c.d_crc.alloc(n * sizeof(uint32_t)));
        {
            Stager st(c.s);
            SVT_TRY(upload(c.d_jobs, jobs, st));
            SVT_TRY(upload_crc_tables(c.d_tables, st));
            SVT_TRY(st.finish());
        }
        SVT_TRY(launch_crc_kernel(bytes, off[n], c.d_jobs.as<crc::Job>(), n, c.d_tables.as<crc::Tables>(), c.d_crc.as<uint32_t>(), nullptr, device, c.s));
        SVT_TRY(d2h_staged(crc, c.d_crc.p, n * sizeof(uint32_t), c.s));
        return SVT_OK;
    });
}

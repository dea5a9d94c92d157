// svt_entry_library.h -- part of the single translation unit svtyper_hip.hip (included there, in order; not a stand-alone header):
// C ABI: svt_bam_scan_libraries_device (include/svtyper_reads.h).  The rounds, the prefix sums, the stop rule, the merge and the
// host scan for whatever is outside the envelope are lw::scan_libraries (svt_reads_library.h), the same code the host twin runs; here
// is only the route's Backend: the arena and the tables in HBM, svt_inflate_kernel and svt_library_kernel.

extern "C++" {

// Destruction order (CallStream, svt_batch_state.h): ~LibraryCall drains the stream, then the buffers are freed, then the stream
// is returned.
struct LibraryCall : CallStream, lw::Backend {
    const bool inflate_on_device;
    GrowBuffer d_arena, d_compressed, d_segments, d_counts, d_caps;
    DeviceInflate inflate;                                   // inflate on the device: kept from round to round
    DevScratch d_rgs, d_blob, d_dense_count, d_dense_first, d_small, d_overflow;
    std::vector<uint8_t> host_arena;                         // inflate on the host: the round's bytes in front of their upload
    uint64_t arena_len = 0;
    uint32_t n_rgs = 0, n_libs = 0, overflow_cap = 0;
    static constexpr size_t kSmallWords = 2 * lw::kMaxLibs + 1;   // read_length, in_lib, and the overflow counter in the low half of a word

    LibraryCall(bool on_device, int device) : inflate_on_device(on_device), inflate(device) {}
    ~LibraryCall() override { drain(); }
    static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
    static double since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); }

    lw::Params params(const GrowBuffer& segments, uint32_t n) const
    {
        lw::Params P{};
        P.arena = d_arena.as<uint8_t>();
        P.arena_len = arena_len;
        P.segments = segments.as<lw::Segment>();
        P.rgs = d_rgs.as<ew::NameRef>();
        P.blob = d_blob.as<uint8_t>();
        P.n_rgs = n_rgs;
        P.n_libs = n_libs;
        P.n_segments = n;
        uint64_t* small = d_small.as<uint64_t>();
        P.T = lw::Tables{d_dense_count.as<uint64_t>(), d_dense_first.as<uint64_t>(), small, small + lw::kMaxLibs, d_overflow.as<lw::Overflow>(),
                         reinterpret_cast<uint32_t*>(small + 2 * lw::kMaxLibs), overflow_cap};
        return P;
    }
    int begin(const std::vector<ew::NameRef>& rgs, const std::vector<uint8_t>& blob, uint32_t n_libs_, uint32_t cap) override
    {
        n_rgs = (uint32_t)rgs.size();
        n_libs = n_libs_;
        overflow_cap = cap;
        const size_t dense = (size_t)n_libs * lw::kDenseKeys * sizeof(uint64_t);
        SVT_TRY(d_dense_count.alloc(dense));
        SVT_TRY(d_dense_first.alloc(dense));
        SVT_TRY(d_small.alloc(kSmallWords * sizeof(uint64_t)));
        SVT_TRY(d_overflow.alloc((size_t)std::max<uint32_t>(cap, 1) * sizeof(lw::Overflow)));
        HIP_TRY(hipMemsetAsync(d_dense_count.p, 0, dense, s));
        HIP_TRY(hipMemsetAsync(d_dense_first.p, 0xFF, dense, s));
        HIP_TRY(hipMemsetAsync(d_small.p, 0, kSmallWords * sizeof(uint64_t), s));
        {
            Stager st(s);
            SVT_TRY(upload(d_rgs, rgs, st));
            SVT_TRY(upload(d_blob, blob, st));
            SVT_TRY(st.finish());
        }
        return SVT_OK;
    }
    int load(const lw::Round& r, std::vector<uint32_t>& member_status, svt_library_scan_stats& S) override
    {
        arena_len = r.set.arena_bytes;
        SVT_TRY(d_arena.need(r.set.arena_bytes + 8));
        if (inflate_on_device) {
            auto t0 = now();
            SVT_TRY(d_compressed.need(r.set.compressed_bytes + 8));
            {
                Stager st(s);
                SVT_TRY(inflate.upload(r.set, d_compressed.d.p, st, r.verify));
                SVT_TRY(st.finish());
            }
            S.upload_s += since(t0);
            t0 = now();
            SVT_TRY(inflate.run(d_compressed.d.p, d_arena.d.p, s, member_status));
            S.inflate_s += since(t0);
        } else {
            auto t0 = now();
            host_arena.resize(r.set.arena_bytes + 8);
            const unsigned nt = std::min<unsigned>(host_threads(), (unsigned)std::max<size_t>(r.set.members.size() / 8, 1));
            bgzf::inflate_members_host(r.set, host_arena.data(), nt, bgzf::Decoder::library, bgzf::Crc::library, r.verify, member_status);
            S.inflate_s += since(t0);
            t0 = now();
            SVT_TRY(h2d_staged(d_arena.d.p, host_arena.data(), r.set.arena_bytes, s));
            S.upload_s += since(t0);
        }
        return SVT_OK;
    }
    int count(const std::vector<lw::Segment>& segments, std::vector<lw::SegCount>& counts) override
    {
        const size_t n = segments.size();
        counts.assign(n, lw::SegCount{});
        if (!n) return SVT_OK;
        SVT_TRY(d_segments.need(n * sizeof(lw::Segment)));
        SVT_TRY(d_counts.need(n * sizeof(lw::SegCount)));
        SVT_TRY(h2d_staged(d_segments.d.p, segments.data(), n * sizeof(lw::Segment), s));
        lw::Params P = params(d_segments, (uint32_t)n);
        P.counts = d_counts.as<lw::SegCount>();
        hipLaunchKernelGGL(svt_library_kernel<false>, dim3((unsigned)n), dim3(kLibraryBlock), 0, s, P);
        HIP_TRY(hipGetLastError());
        SVT_TRY(d2h_staged(counts.data(), d_counts.d.p, n * sizeof(lw::SegCount), s));
        return SVT_OK;
    }
    int accumulate(const std::vector<lw::Segment>&, const std::vector<lw::SegCaps>& caps) override
    {
        const size_t n = caps.size();                           // (the segments are the count pass's, still in HBM)
        if (!n) return SVT_OK;
        SVT_TRY(d_caps.need(n * sizeof(lw::SegCaps)));
        SVT_TRY(h2d_staged(d_caps.d.p, caps.data(), n * sizeof(lw::SegCaps), s));
        lw::Params P = params(d_segments, (uint32_t)n);
        P.caps = d_caps.as<lw::SegCaps>();
        hipLaunchKernelGGL(svt_library_kernel<true>, dim3((unsigned)n), dim3(kLibraryBlock), 0, s, P);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        return SVT_OK;
    }
    int finish(lw::HostTables& T) override
    {
        const size_t dense = (size_t)n_libs * lw::kDenseKeys;
        T.n_libs = n_libs;
        T.dense_count.resize(dense);
        T.dense_first.resize(dense);
        std::vector<uint64_t> small(kSmallWords);
        SVT_TRY(d2h_staged(small.data(), d_small.p, kSmallWords * sizeof(uint64_t), s));
        T.read_length.assign(small.begin(), small.begin() + lw::kMaxLibs);
        T.in_lib.assign(small.begin() + lw::kMaxLibs, small.begin() + 2 * lw::kMaxLibs);
        T.overflow_n = (uint32_t)small[2 * lw::kMaxLibs];
        SVT_TRY(d2h_staged(T.dense_count.data(), d_dense_count.p, dense * sizeof(uint64_t), s));
        SVT_TRY(d2h_staged(T.dense_first.data(), d_dense_first.p, dense * sizeof(uint64_t), s));
        T.overflow.resize(std::min(T.overflow_n, overflow_cap));
        if (!T.overflow.empty()) SVT_TRY(d2h_staged(T.overflow.data(), d_overflow.p, T.overflow.size() * sizeof(lw::Overflow), s));
        return SVT_OK;
    }
};

}  // extern "C++"

int svt_bam_scan_libraries_device(const svt_bam* bam, uint32_t n_libs, const uint32_t* rg_counts, const char* const* read_groups, int64_t num_samp,
                                  uint64_t round_bytes, int inflate_on_device, int device, svt_library_scan* out, svt_library_scan_stats* stats)
{
    return guarded([&]() -> int {
        SVT_TRY(select_device(device));
        VerifyScope verify_scope(bam);
        LibraryCall c(inflate_on_device != 0, device);
        SVT_TRY(c.take());
        return lw::scan_libraries(bam, n_libs, rg_counts, read_groups, num_samp, round_bytes, c, out, stats);
    });
}

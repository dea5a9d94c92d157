// svt_entry_bam_first.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_bam_sort.h; not a stand-alone header): first occurrences of a BAM record stream on the device.  The stream and the
// offset table go up once; svt_bam_first_hash_kernel checks every record and writes (hash, index); the pairs go through the
// call's RadixSort (svt_entry_radix_sort.h: the one sort, not a copy of it); svt_bam_first_mark_kernel compares
// neighbours inside runs of equal hashes and counts; keep and the workgroups' counts come down.  C ABI: svt_bam_first_device,
// svt_bam_first_last_times (include/svtyper_reads.h); the host twin is svt_bam_first_host (svt_reads_bam_sort_entries.h).

extern "C++" {

// the kernels of the calling thread's last svt_bam_first_device, from HIP events, and the call's wall time
static thread_local svt_bam_first_times g_bam_first_times;

struct BamFirstCall : OrderedCall {                          // (svt_entry_deflate.h; destruction order: CallStream, svt_batch_state.h)
    DevScratch d_rec_off, d_bad, d_keep, d_kept;
    RadixSort sort;                                          // (a member, so freed behind drain())
    ~BamFirstCall() { drain(); }
};

static int svt_bam_first_device_impl(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept,
                                     uint64_t* bad_record, uint32_t hash_bits, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_bam_first_times = svt_bam_first_times();
    if ((len && !bytes) || !rec_off || (n && !keep) || !n_kept || !bad_record) return fail(SVT_ERR_INVALID, "null argument");
    if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_first: too many records in one call (< 2^32)");
    if (hash_bits < 1 || hash_bits > 64) return fail(SVT_ERR_INVALID, "svt_bam_first: hash_bits is 1..64");
    for (uint64_t i = 0; i < n; ++i)
        if (rec_off[i] > rec_off[i + 1]) return fail(SVT_ERR_INVALID, "svt_bam_first: rec_off must not decrease");
    *n_kept = 0;
    *bad_record = 0;
    SVT_TRY(select_device(device));
    if (n == 0) return SVT_OK;
    if (len == 0) {                                 // (no bytes: the first record is no record)
        *bad_record = 1;
        return SVT_OK;
    }
    BamFirstCall c;
    SVT_TRY(c.begin(bytes, len));
    unsigned grid = 0;
    SVT_TRY(c.d_rec_off.alloc((n + 1) * sizeof(uint64_t)));
    SVT_TRY(h2d_staged(c.d_rec_off.p, rec_off, (n + 1) * sizeof(uint64_t), c.s));
    SVT_TRY(c.sort.room(n));
    SVT_TRY(c.sort.key_grid(n, device, &grid));
    SVT_TRY(c.d_bad.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(c.d_bad.p, 0xFF, sizeof(unsigned long long), c.s));          // kFirstNoBad
    size_t e[4] = {};
    SVT_TRY(c.mark(&e[0]));
    hipLaunchKernelGGL(svt_bam_first_hash_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_rec_off.as<uint64_t>(), n,
                       bfr::hash_mask(hash_bits), c.sort.keys(), c.sort.idx(), c.sort.part_and(), c.sort.part_or(), c.d_bad.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[1]));
    unsigned long long bad = kFirstNoBad;
    SVT_TRY(d2h_staged(&bad, c.d_bad.p, sizeof bad, c.s));
    SVT_TRY(c.sort.combine(c));
    SVT_TRY(c.between(e[0], e[1], &g_bam_first_times.hash_kernel_s));
    if (bad != kFirstNoBad) {
        if (bad >= n) return fail(SVT_ERR_HIP, "svt_bam_first_hash_kernel: the record it refuses is none of the stream's");
        *bad_record = bad + 1;
        g_bam_first_times.total_s = seconds_since(t0);
        return SVT_OK;
    }
    SVT_TRY(c.sort.passes(c, device));
    SVT_TRY(c.d_keep.alloc(n));
    SVT_TRY(c.d_kept.alloc(grid * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c.d_keep.p, 0xFF, n, c.s));       // (a record the mark kernel did not reach shows below)
    SVT_TRY(c.mark(&e[2]));
    hipLaunchKernelGGL(svt_bam_first_mark_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_rec_off.as<uint64_t>(), n,
                       c.sort.sorted_keys(), c.sort.sorted_idx(), c.d_keep.as<uint8_t>(), c.d_kept.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e[3]));
    std::vector<uint32_t> kept(grid);
    SVT_TRY(d2h_staged(keep, c.d_keep.p, n, c.s));
    SVT_TRY(d2h_staged(kept.data(), c.d_kept.p, grid * sizeof(uint32_t), c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    svt_bam_first_times& t = g_bam_first_times;
    SVT_TRY(c.sort.times(c, &t.passes, &t.histogram_kernel_s, &t.scan_kernel_s, &t.scatter_kernel_s));
    SVT_TRY(c.between(e[2], e[3], &g_bam_first_times.mark_kernel_s));
    // every record got its 0 or 1 and the workgroups' counts are their sum, or the answer is not the kernels'
    uint64_t reduced = 0, summed = 0;
    for (unsigned g = 0; g < grid; ++g) reduced += kept[g];
    for (uint64_t i = 0; i < n; ++i) {
        if (keep[i] > 1) return fail(SVT_ERR_HIP, "svt_bam_first_mark_kernel: a record was not decided");
        summed += keep[i];
    }
    if (reduced != summed || !keep[0]) return fail(SVT_ERR_HIP, "svt_bam_first_mark_kernel: the count is not the sum of keep");
    *n_kept = reduced;
    g_bam_first_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_bam_first_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t* n_kept, uint64_t* bad_record,
                         uint32_t hash_bits, int device)
{
    return guarded([&] { return svt_bam_first_device_impl(bytes, len, rec_off, n, keep, n_kept, bad_record, hash_bits, device); });
}

int svt_bam_first_last_times(svt_bam_first_times* times) { return guarded([&] { return last_times(times, g_bam_first_times); }); }

// svt_entry_radix_sort.h -- part of the single translation unit svtyper_hip.hip (included there, in order, in front of
// svt_entry_bam_sort.h; not a stand-alone header): the host side of svt_radix_sort_kernel.h, one object.  Its users are the
// record sort (svt_entry_bam_sort.h), the first-occurrence pass (svt_entry_bam_first.h) and the index fold's run sort
// (svt_entry_bam_index.h).  Each launches a key kernel of its own over keys() / idx() / part_and() / part_or() and then asks:
// combine, passes (or order), sorted_keys / sorted_idx, times.  Everything runs on the stream the caller passes and touches
// nothing else of the caller's call; no g_*_times is written here.

extern "C++" {

// A stable sort of n (64-bit key, 32-bit index) pairs on the device.  Release rule: a RadixSort is a MEMBER of the struct that
// derives from the caller's CallStream and whose destructor calls drain() (destruction order: CallStream, svt_batch_state.h), so
// its buffers are freed behind the drain and in front of the stream's return, like every other DevScratch of that call.
struct RadixSort {
    // keys() / idx() for `capacity` pairs
    int room(uint64_t capacity)
    {
        SVT_TRY(d_keys[0].alloc(capacity * sizeof(uint64_t)));
        return d_idx[0].alloc(capacity * sizeof(uint32_t));
    }
    // n pairs (n <= capacity) are what a key kernel is about to write: the grid to launch it with, part_and() / part_or() for it
    int key_grid(uint64_t n, int device, unsigned* grid) { return key_grid(n, n, device, grid); }
    // the same for a key kernel that walks `work` elements to write its n pairs (a compaction: svt_entry_vcf_group.h)
    int key_grid(uint64_t n, uint64_t work, int device, unsigned* grid)
    {
        n_ = n;
        grid_ = *grid = lines_grid((work + kSortBlock - 1) / kSortBlock, device);
        SVT_TRY(d_and.alloc(grid_ * sizeof(uint64_t)));
        return d_or.alloc(grid_ * sizeof(uint64_t));
    }
    uint64_t* keys() const { return d_keys[0].as<uint64_t>(); }
    uint32_t* idx() const { return d_idx[0].as<uint32_t>(); }
    uint64_t* part_and() const { return d_and.as<uint64_t>(); }
    uint64_t* part_or() const { return d_or.as<uint64_t>(); }

    // the key kernel's partials brought down (the stream is synchronised) and combined into the keys' AND / OR
    int combine(TimedCallStream& c)
    {
        std::vector<uint64_t> ands(grid_), ors(grid_);
        SVT_TRY(d2h_staged(ands.data(), d_and.p, grid_ * sizeof(uint64_t), c.s));
        SVT_TRY(d2h_staged(ors.data(), d_or.p, grid_ * sizeof(uint64_t), c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
        key_and = ~0ull, key_or = 0;
        for (unsigned g = 0; g < grid_; ++g) {
            key_and &= ands[g];
            key_or |= ors[g];
        }
        return SVT_OK;
    }
    // instead of key_grid and combine, for n pairs the caller made on the host and put into keys() / idx()
    void given(uint64_t n, uint64_t all_and, uint64_t all_or) { n_ = n, key_and = all_and, key_or = all_or; }

    // The radix passes, launched on c.s: one histogram, scan and scatter per 8-bit digit in which the keys differ, least
    // significant first (no digit differs: no pass).  Behind them sorted_keys() / sorted_idx() hold the pairs in stable order by key.
    int passes(TimedCallStream& c, int device)
    {
        const uint64_t n = n_, differ = n ? key_and ^ key_or : 0;
        uint32_t shifts[8], count = 0;
        for (uint32_t d = 0; d < 8; ++d)
            if (differ >> (8 * d) & 255) shifts[count++] = 8 * d;
        src_ = 0;
        at_.assign(4 * count, 0);
        if (count == 0) return SVT_OK;
        const uint32_t n_tiles = (uint32_t)((n + kSortTile - 1) / kSortTile);
        const unsigned grid = lines_grid(n_tiles, device);
        SVT_TRY(d_keys[1].alloc(n * sizeof(uint64_t)));
        SVT_TRY(d_idx[1].alloc(n * sizeof(uint32_t)));
        SVT_TRY(d_hist.alloc((uint64_t)n_tiles * 256 * sizeof(uint32_t)));
        for (uint32_t p = 0; p < count; ++p) {
            SVT_TRY(c.mark(&at_[4 * p]));
            hipLaunchKernelGGL(svt_bam_histogram_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, d_keys[src_].as<uint64_t>(), n, n_tiles, shifts[p],
                               d_hist.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            SVT_TRY(c.mark(&at_[4 * p + 1]));
            hipLaunchKernelGGL(svt_bam_scan_kernel, dim3(1), dim3(kSortBlock), 0, c.s, d_hist.as<uint32_t>(), (uint64_t)n_tiles * 256);
            HIP_TRY(hipGetLastError());
            SVT_TRY(c.mark(&at_[4 * p + 2]));
            hipLaunchKernelGGL(svt_bam_scatter_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, d_keys[src_].as<uint64_t>(), d_idx[src_].as<uint32_t>(), n, n_tiles,
                               shifts[p], d_hist.as<uint32_t>(), d_keys[src_ ^ 1].as<uint64_t>(), d_idx[src_ ^ 1].as<uint32_t>());
            HIP_TRY(hipGetLastError());
            SVT_TRY(c.mark(&at_[4 * p + 3]));
            src_ ^= 1;
        }
        return SVT_OK;
    }
    const uint64_t* sorted_keys() const { return d_keys[src_].as<uint64_t>(); }
    const uint32_t* sorted_idx() const { return d_idx[src_].as<uint32_t>(); }

    // passes, then order[j]: the index that comes j-th in stable order by key, brought down and checked (the stream is synchronised
    // where there was a pass)
    int order(TimedCallStream& c, std::vector<uint32_t>& order, int device)
    {
        order.resize(n_);
        SVT_TRY(passes(c, device));
        if (at_.empty()) {                          // every key is the same one: the order of arrival
            for (uint64_t i = 0; i < n_; ++i) order[i] = (uint32_t)i;
            return SVT_OK;
        }
        SVT_TRY(d2h_staged(order.data(), sorted_idx(), n_ * sizeof(uint32_t), c.s));
        HIP_TRY(hipStreamSynchronize(c.s));
        // the kernels' order is a permutation or it is not theirs: what the gather and the callers rely on
        std::vector<uint8_t> seen(n_, 0);
        for (uint64_t j = 0; j < n_; ++j) {
            if (order[j] >= n_ || seen[order[j]]) return fail(SVT_ERR_HIP, "svt_bam_scatter_kernel: the order is no permutation");
            seen[order[j]] = 1;
        }
        return SVT_OK;
    }

    // what the passes were, once c.s has passed their marks, handed to the caller for its own *_times: their number, and each
    // kernel's seconds over all passes ADDED to its sum (the three may be one sum: the index fold's sort_kernel_s)
    int times(TimedCallStream& c, uint32_t* count, double* histogram_s, double* scan_s, double* scatter_s) const
    {
        *count = (uint32_t)(at_.size() / 4);
        for (uint32_t p = 0; p < *count; ++p) {
            SVT_TRY(c.between(at_[4 * p], at_[4 * p + 1], histogram_s));
            SVT_TRY(c.between(at_[4 * p + 1], at_[4 * p + 2], scan_s));
            SVT_TRY(c.between(at_[4 * p + 2], at_[4 * p + 3], scatter_s));
        }
        return SVT_OK;
    }

    uint64_t key_and = ~0ull, key_or = 0;           // of the n keys: combine's or given's

private:
    DevScratch d_keys[2], d_idx[2], d_and, d_or, d_hist;
    uint64_t n_ = 0;
    unsigned grid_ = 0;
    int src_ = 0;
    std::vector<size_t> at_;                        // four marks per pass
};

}  // extern "C++"

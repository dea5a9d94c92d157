// svt_entry_bam_sort.h -- part of the single translation unit svtyper_hip.hip (included there, in order, behind
// svt_entry_radix_sort.h; not a stand-alone header): BAM records as spans on the device.  What is this header's: the span table
// (keys_resident: svt_bam_keys_kernel writes spans, keys and their AND / OR per workgroup), the record sort over the call's
// RadixSort (sort_resident: svt_entry_radix_sort.h has the passes, their buffers and their times), the argument checks and the
// caller's arrays.  What it shares lives in svt_entry_deflate.h: the upload (OrderedCall::begin), the gather behind the header
// copy (gather_resident<svt_bam_span>), the members from bsr::cut_members' boundaries (deflate_members), the marks that time the
// kernels.  C ABI: svt_bam_spans_device, svt_bam_sort_order_device, svt_bam_sorted_bgzf_device, svt_bam_sort_last_times
// (include/svtyper_reads.h).  The one-call entry's body takes a hook that runs behind the members while its tables are resident:
// svt_entry_bam_index.h's CSI fold.

extern "C++" {

// the kernels of the calling thread's last call here, from HIP events, and the call's wall time
static thread_local svt_bam_sort_times g_bam_sort_times;

struct BamSortCall : OrderedCall {                           // (svt_entry_deflate.h; destruction order: CallStream, svt_batch_state.h)
    DevScratch d_rec_off, d_spans;
    RadixSort sort;                                          // (svt_entry_radix_sort.h: a member, so freed behind drain())
    ~BamSortCall() { drain(); }
};

// c.d_stream[0, len) and the caller's rec_off -> the span table in c.d_spans and in `table`, keys and indices in c.sort with the
// AND and the OR of the keys
static int keys_resident(BamSortCall& c, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, std::vector<svt_bam_span>& table, int device)
{
    table.clear();
    if (n == 0) return SVT_OK;
    unsigned grid = 0;
    SVT_TRY(c.d_rec_off.alloc((n + 1) * sizeof(uint64_t)));
    SVT_TRY(h2d_staged(c.d_rec_off.p, rec_off, (n + 1) * sizeof(uint64_t), c.s));
    SVT_TRY(c.d_spans.alloc(n * sizeof(svt_bam_span)));
    SVT_TRY(c.sort.room(n));
    SVT_TRY(c.sort.key_grid(n, device, &grid));
    size_t e0 = 0, e1 = 0;
    SVT_TRY(c.mark(&e0));
    hipLaunchKernelGGL(svt_bam_keys_kernel, dim3(grid), dim3(kSortBlock), 0, c.s, c.d_stream.as<uint8_t>(), len, c.d_rec_off.as<uint64_t>(), n, n_ref,
                       c.d_spans.as<svt_bam_span>(), c.sort.keys(), c.sort.idx(), c.sort.part_and(), c.sort.part_or());
    HIP_TRY(hipGetLastError());
    SVT_TRY(c.mark(&e1));
    table.resize(n);
    SVT_TRY(d2h_staged(table.data(), c.d_spans.p, n * sizeof(svt_bam_span), c.s));
    SVT_TRY(c.sort.combine(c));
    SVT_TRY(c.between(e0, e1, &g_bam_sort_times.keys_kernel_s));
    // the kernel's table is the caller's offsets or it is not theirs: what the gather relies on
    for (uint64_t i = 0; i < n; ++i)
        if (table[i].off != rec_off[i] || (table[i].len && (table[i].off > len || table[i].len > len - table[i].off)))
            return fail(SVT_ERR_HIP, "svt_bam_keys_kernel: the spans are not the offset table's");
    return SVT_OK;
}

// the pairs of c.sort -> order[j]: the index that comes j-th in stable order by key; the passes' times into g_bam_sort_times
static int sort_resident(BamSortCall& c, std::vector<uint32_t>& order, int device)
{
    SVT_TRY(c.sort.order(c, order, device));
    svt_bam_sort_times& t = g_bam_sort_times;
    return c.sort.times(c, &t.passes, &t.histogram_kernel_s, &t.scan_kernel_s, &t.scatter_kernel_s);
}

static int svt_bam_spans_device_impl(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, svt_bam_span* spans,
                                     uint64_t* key_and, uint64_t* key_or, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_bam_sort_times = svt_bam_sort_times();
    if ((len && !bytes) || !rec_off || (n && !spans)) return fail(SVT_ERR_INVALID, "null argument");
    if (n_ref < 0) return fail(SVT_ERR_INVALID, "svt_bam_spans: n_ref is negative");
    if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_spans: too many records in one call (< 2^32)");
    SVT_TRY(select_device(device));
    BamSortCall c;
    SVT_TRY(c.begin(bytes, len));
    std::vector<svt_bam_span> table;
    SVT_TRY(keys_resident(c, len, rec_off, n, n_ref, table, device));
    if (n) std::memcpy(spans, table.data(), n * sizeof(svt_bam_span));
    if (key_and) *key_and = c.sort.key_and;
    if (key_or) *key_or = c.sort.key_or;
    g_bam_sort_times.total_s = seconds_since(t0);
    return SVT_OK;
}

static int svt_bam_sort_order_device_impl(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_bam_sort_times = svt_bam_sort_times();
    if ((n && (!spans || !perm)) || !bad_record || !bad_kind) return fail(SVT_ERR_INVALID, "null argument");
    if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_sort_order: too many records in one call (< 2^32)");
    SVT_TRY(select_device(device));
    *bad_record = bsr::first_bad(spans, n, *bad_kind);
    if (*bad_record || n == 0) return SVT_OK;
    BamSortCall c;
    SVT_TRY(c.take());
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> idx(n), order;
    uint64_t a = ~0ull, o = 0;
    for (uint64_t i = 0; i < n; ++i) {
        keys[i] = spans[i].key;
        idx[i] = (uint32_t)i;
        a &= keys[i];
        o |= keys[i];
    }
    SVT_TRY(c.sort.room(n));
    {
        Stager st(c.s);
        SVT_TRY(st.copy(c.sort.keys(), keys.data(), n * sizeof(uint64_t)));
        SVT_TRY(st.copy(c.sort.idx(), idx.data(), n * sizeof(uint32_t)));
        SVT_TRY(st.finish());
    }
    c.sort.given(n, a, o);
    SVT_TRY(sort_resident(c, order, device));
    for (uint64_t j = 0; j < n; ++j) perm[j] = order[j];
    g_bam_sort_times.total_s = seconds_since(t0);
    return SVT_OK;
}

// what svt_bam_sorted_bgzf_csi_device (svt_entry_bam_index.h) does behind the members, while the call's tables are resident:
// (the call, whether the records were gathered, the number of members)
using BamFoldHook = std::function<int(BamSortCall&, bool, uint64_t)>;

static int svt_bam_sorted_bgzf_device_impl(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, int sort, uint32_t mode,
                                           uint8_t* out, uint64_t capacity, uint64_t* out_off, uint64_t member_capacity, uint64_t* n_members,
                                           uint64_t* member_start, svt_bam_span* spans, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, int device,
                                           const BamFoldHook* behind = nullptr)
{
    const auto t0 = std::chrono::steady_clock::now();
    g_bam_sort_times = svt_bam_sort_times();
    g_deflate_times = svt_deflate_times();
    SVT_TRY(deflate_check_mode("svt_bam_sorted_bgzf", mode));
    if (!rec_off || !out_off || !n_members || !member_start || !bad_record || !bad_kind || (len && (!bytes || !out)) || (n && (!spans || !perm)))
        return fail(SVT_ERR_INVALID, "null argument");
    if (n_ref < 0) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf: n_ref is negative");
    if (n >> 32) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf: too many records in one call (< 2^32)");
    if (rec_off[0] > len || rec_off[n] != len) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf: the records end where the bytes end");
    for (uint64_t i = 0; i < n; ++i)
        if (rec_off[i] > rec_off[i + 1]) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf: rec_off must not decrease");
    *n_members = 0;
    *bad_record = 0;
    *bad_kind = 0;
    out_off[0] = 0;
    member_start[0] = 0;
    SVT_TRY(select_device(device));
    if (len == 0) return SVT_OK;
    BamSortCall c;
    SVT_TRY(c.begin(bytes, len));
    const uint64_t header_len = rec_off[0];
    std::vector<svt_bam_span> table;
    SVT_TRY(keys_resident(c, len, rec_off, n, n_ref, table, device));
    const uint8_t* d_written = c.d_stream.as<uint8_t>();
    if (sort) {
        *bad_record = bsr::first_bad(table.data(), n, *bad_kind);
        if (*bad_record) return SVT_OK;
        std::vector<uint32_t> order;
        SVT_TRY(sort_resident(c, order, device));
        std::vector<uint64_t> dst_off(n);
        uint64_t at = header_len;
        for (uint64_t j = 0; j < n; ++j) {
            perm[j] = order[j];
            dst_off[j] = at;
            at += table[order[j]].len;
        }
        if (at != len) return fail(SVT_ERR_INTERNAL, "svt_bam_sorted_bgzf: the records' lengths do not sum to the stream's");
        SVT_TRY(c.d_sorted.alloc(len));
        if (header_len) HIP_TRY(hipMemcpyAsync(c.d_sorted.p, c.d_stream.p, header_len, hipMemcpyDeviceToDevice, c.s));
        SVT_TRY(gather_resident(c, c.d_stream.as<uint8_t>(), len, c.d_spans.as<svt_bam_span>(), n, perm, dst_off, c.d_sorted.as<uint8_t>(), len,
                                &g_bam_sort_times.gather_kernel_s, device));
        d_written = c.d_sorted.as<uint8_t>();
        for (uint64_t j = 0; j < n; ++j) {
            spans[j] = table[order[j]];
            spans[j].off = dst_off[j];
        }
    } else {
        for (uint64_t j = 0; j < n; ++j) {
            spans[j] = table[j];
            perm[j] = j;
        }
    }
    std::vector<uint64_t> start;
    bsr::cut_members(header_len, n, [&](uint64_t j) { return spans[j].len; }, start);        // cut where bgzf.BgzfWriter cuts
    const uint64_t members = start.size() - 1;
    if (members > member_capacity) return fail(SVT_ERR_INVALID, "svt_bam_sorted_bgzf: member_capacity is below the number of members");
    std::memcpy(member_start, start.data(), start.size() * sizeof(uint64_t));
    SVT_TRY(deflate_members(c, "svt_bam_sorted_bgzf", d_written, start.data(), members, out, capacity, out_off, mode, device));
    *n_members = members;
    if (behind) SVT_TRY((*behind)(c, sort != 0, members));
    g_bam_sort_times.total_s = g_deflate_times.total_s = seconds_since(t0);
    return SVT_OK;
}

}  // extern "C++"

int svt_bam_spans_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, svt_bam_span* spans, uint64_t* key_and,
                         uint64_t* key_or, int device)
{
    return guarded([&] { return svt_bam_spans_device_impl(bytes, len, rec_off, n, n_ref, spans, key_and, key_or, device); });
}

int svt_bam_sort_order_device(const svt_bam_span* spans, uint64_t n, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    return guarded([&] { return svt_bam_sort_order_device_impl(spans, n, perm, bad_record, bad_kind, device); });
}

int svt_bam_sorted_bgzf_device(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, int32_t n_ref, int sort, uint32_t mode, uint8_t* out,
                               uint64_t capacity, uint64_t* out_off, uint64_t member_capacity, uint64_t* n_members, uint64_t* member_start,
                               svt_bam_span* spans, uint64_t* perm, uint64_t* bad_record, uint32_t* bad_kind, int device)
{
    return guarded([&] {
        return svt_bam_sorted_bgzf_device_impl(bytes, len, rec_off, n, n_ref, sort, mode, out, capacity, out_off, member_capacity, n_members, member_start,
                                               spans, perm, bad_record, bad_kind, device);
    });
}

int svt_bam_sort_last_times(svt_bam_sort_times* times) { return guarded([&] { return last_times(times, g_bam_sort_times); }); }

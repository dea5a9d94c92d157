// svt_vcf_group_kernel.h -- svt_vcf_group.h on the device (gfx950): the body lines of a VCF in HBM under their line table -> one
// svt_group_line per line and, for a regular file, the plan.  The join over the whole file is "hash, sort (hash,
// index), confirm by bytes inside a run of equal hashes", as svt_bam_first_kernel.h's; the sort is svt_radix_sort_kernel.h's.
//
//   svt_group_scan_kernel     ONE LANE PER LINE: group::scan_line, the host twin's source.  bnd[i] = 1 for a BND line the rule
//                             decided, emit[i] = 1 for any other line it decided; the smallest line the script dies ON goes to
//                             status->fatal (one 64-bit integer atomic minimum), a marked line sets status->any_slow (one
//                             flag: reduced over the wavefront's lanes, then one OR per wavefront that met one; the match
//                             kernel's `irregular` likewise).  Why a lane and not a wavefront per line:
//                             profiles/group_kernel_resources.txt
//   (bnd is scanned by svt_bam_scan_kernel: where a BND line stands among the BND lines)
//   svt_group_compact_kernel  keys[c] = the masked FNV-1a of the ID of the c-th BND line, idx[c] = its line; ends in
//                             radix_store_and_or, like every key kernel of the sort
//   (the radix passes)
//   svt_group_match_kernel    one lane per sorted position: backwards in its run of equal hashes for an EARLIER position with its
//                             own ID's bytes (a duplicate ID: not regular); a binary search of the sorted hashes for its MATEID's
//                             hash, then forwards in that run for the line whose ID is the MATEID's bytes.  The mate must be
//                             another line and name this one back, or the file is not regular.  A line whose mate stands in
//                             front of it is the second of a pair: emit = 2, mate[i] = the first; it dies there if either lacks
//                             SVT_GROUP_CI
//   (emit is scanned: where a line's entries go)
//   svt_group_plan_kernel     the entries of every line in front of the fatal one
// Every load of the text goes through a record whose spans group::spans_inside has checked against the text's length, every index
// that came out of the sort against the line count, every store against the element count.  No workgroup waits for another, no
// float atomics, no inline assembly, no scratch memory.
#ifndef SVT_VCF_GROUP_KERNEL_H
#define SVT_VCF_GROUP_KERNEL_H

#include "svt_radix_sort_kernel.h"
#include "svt_vcf_group.h"

namespace svt {

constexpr unsigned long long kGroupNoFatal = ~0ull;

struct GroupStatus {
    unsigned long long fatal;                       // the smallest 0-based line the script dies on
    uint32_t any_slow, irregular;
};

// bnd and emit hold n + 1 elements, zeroed: the last one is where their scans leave the totals
__global__ __launch_bounds__(kSortBlock) void svt_group_scan_kernel(const uint8_t* __restrict__ text, uint64_t len, const svt_tbx_line* __restrict__ lines,
                                                                    uint64_t n, const uint8_t* __restrict__ format_table, uint32_t format_len,
                                                                    svt_group_line* __restrict__ records, uint32_t* __restrict__ bnd,
                                                                    uint32_t* __restrict__ emit, GroupStatus* __restrict__ status)
{
    bool slow = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSortBlock) {
        const uint64_t off = lines[i].off, size = lines[i].len;
        svt_group_line r = svt_group_line();
        if (off <= len && size <= len - off) r = group::scan_line(text + off, off, size, format_table, format_len);
        else r.slow = SVT_GROUP_SLOW_HEAD;          // (a table that is not the text's: the host has checked that it is)
        records[i] = r;
        const bool is_bnd = !r.slow && (r.flags & SVT_GROUP_BND);
        bnd[i] = is_bnd ? 1u : 0u;
        emit[i] = !r.slow && !is_bnd ? 1u : 0u;
        slow = slow || r.slow;
        if (r.bad) atomicMin(&status->fatal, (unsigned long long)i);
    }
    if (__any(slow) && (threadIdx.x & 63) == 0) atomicOr(&status->any_slow, 1u);     // (behind the loop: every lane is here)
}

// at: the exclusive scan of bnd, n + 1 elements
__global__ __launch_bounds__(kSortBlock) void svt_group_compact_kernel(const uint8_t* __restrict__ text, uint64_t len,
                                                                       const svt_group_line* __restrict__ records, uint64_t n,
                                                                       const uint32_t* __restrict__ at, uint64_t n_bnd, uint64_t mask,
                                                                       uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                       uint64_t* __restrict__ key_and, uint64_t* __restrict__ key_or)
{
    uint64_t a = ~0ull, o = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kSortBlock) {
        const uint32_t c = at[i];
        if (at[i + 1] == c || c >= n_bnd) continue;
        const svt_group_line r = records[i];
        const uint64_t h = group::spans_inside(r, len) ? group::id_hash(text + r.off, r.id_b, r.id_n, mask) : 0;
        keys[c] = h;
        idx[c] = (uint32_t)i;
        a &= h;
        o |= h;
    }
    radix_store_and_or(a, o, key_and, key_or);
}

// keys / idx: the (ID hash, line) pairs of the n_bnd BND lines in stable order by hash
__global__ __launch_bounds__(kSortBlock) void svt_group_match_kernel(const uint8_t* __restrict__ text, uint64_t len,
                                                                     const svt_group_line* __restrict__ records, uint64_t n,
                                                                     const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n_bnd,
                                                                     uint64_t mask, uint32_t* __restrict__ emit, uint32_t* __restrict__ mate,
                                                                     GroupStatus* __restrict__ status)
{
    bool irregular = false;
    for (uint64_t j = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; j < n_bnd; j += (uint64_t)gridDim.x * kSortBlock) {
        const uint64_t i = idx[j];
        if (i >= n) {
            irregular = true;
            continue;
        }
        const svt_group_line r = records[i];
        if (!group::spans_inside(r, len)) {
            irregular = true;
            continue;
        }
        const uint8_t* p = text + r.off;
        const uint64_t h = keys[j];
        for (uint64_t b = j; b > 0 && keys[b - 1] == h; --b) {         // another BND line with this ID
            const uint64_t e = idx[b - 1];
            if (e >= n) continue;
            const svt_group_line o = records[e];
            if (group::spans_inside(o, len) && group::same_bytes(p + r.id_b, r.id_n, text + o.off + o.id_b, o.id_n)) {
                irregular = true;
                break;
            }
        }
        if (!(r.flags & SVT_GROUP_HAS_MATE)) continue;
        const uint64_t want = group::id_hash(p, r.mate_b, r.mate_n, mask);
        uint64_t lo = 0, hi = n_bnd;                                    // the first position whose hash is not below `want`
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (keys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        for (uint64_t f = lo; f < n_bnd && keys[f] == want; ++f) {
            const uint64_t m = idx[f];
            if (m >= n) continue;
            const svt_group_line o = records[m];
            if (!group::spans_inside(o, len) || !group::same_bytes(p + r.mate_b, r.mate_n, text + o.off + o.id_b, o.id_n)) continue;
            if (m == i || !(o.flags & SVT_GROUP_HAS_MATE) || !group::same_bytes(text + o.off + o.mate_b, o.mate_n, p + r.id_b, r.id_n))
                irregular = true;
            else if (m < i) {
                emit[i] = 2;
                mate[i] = (uint32_t)m;
                if (!(o.flags & SVT_GROUP_CI) || !(r.flags & SVT_GROUP_CI)) atomicMin(&status->fatal, (unsigned long long)i);
            }
            break;
        }
    }
    if (__any(irregular) && (threadIdx.x & 63) == 0) atomicOr(&status->irregular, 1u);     // (behind the loop: every lane is here)
}

// at: the exclusive scan of emit, n + 1 elements; `fatal`: the first line that writes nothing (n: none); plan holds `capacity`
__global__ __launch_bounds__(kSortBlock) void svt_group_plan_kernel(const uint32_t* __restrict__ at, const uint32_t* __restrict__ mate, uint64_t n,
                                                                    uint64_t fatal, svt_group_out* __restrict__ plan, uint64_t capacity)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x; i < n && i < fatal; i += (uint64_t)gridDim.x * kSortBlock) {
        const uint64_t to = at[i], count = at[i + 1] - at[i];
        if (count == 1 && to < capacity) plan[to] = svt_group_out{(uint32_t)i, (uint32_t)i};
        if (count == 2 && to + 1 < capacity && mate[i] < n) {
            plan[to] = svt_group_out{mate[i], mate[i]};
            plan[to + 1] = svt_group_out{(uint32_t)i, mate[i]};
        }
    }
}

}  // namespace svt

#endif  // SVT_VCF_GROUP_KERNEL_H

// svt_wg_parts.h -- what the kernels over canonical records share around their record loops
// Internal header of libsvtyper_hip.so (included by svt_stream_kernel.h).
//
// svt_stream_kernel (one lane per unit), svt_split_kernel (K lanes per unit) and svt_coop_kernel (producer and consumer waves)
// are one family: one StreamArgs, one LDS table layout (kSPm ... kSBins), one unit epilogue, one result-record form.  They
// differ in how a block's records reach the lane that sums them; this file holds the rest, once:
//
//   * wg_units       which units the workgroup owns (consecutive ones, or a chunk of the window permutation);
//   * stage_tables   prob_mapq and its half, the weight columns, the bins (one library / the window's, with its WinLibs / the
//                    general mode's descriptors) and the log10 table into LDS;
//   * the tile entry {first record, records, sub2, flags} the kernels for small launches keep per sorted position
//                    (the sort itself: wg_sort_units, svt_ring_engine.h);
//   * result_destination   the tail of every epilogue (with result96_tag, svt_ring_engine.h);
//   * tally_epilogue the epilogue of a unit whose tallies wait in LDS.
//
// Everything is __forceinline__ and keeps the statement order the kernels had when they carried these parts themselves: the
// kernels are sensitive to hoisting (svt_stream_kernel.h, svt_ring_engine.h: store_result_records_through_ring).
#ifndef SVT_WG_PARTS_H
#define SVT_WG_PARTS_H

#include "svt_ring_engine.h"

namespace svt {

// LDS layout of the streaming kernel, absolute byte addresses (the kernel has no static LDS, so the dynamic
// segment starts at 0 -- checked at run time): the one-library record consumer turns every field of a record
// into an LDS address with one instruction and the table base as the ds_read's immediate offset.
constexpr uint32_t kSPm = 0;                          // double[256]  prob_mapq(q)                      (utils.py:74-75)
constexpr uint32_t kSPmHalf = kSPm + 256 * 8;         // double[256]  prob_mapq(q) / 2 (exact: a power-of-two scaling)
constexpr uint32_t kSWtab = kSPmHalf + 256 * 8;       // kSingleLds: double w_alt[32], w_ref[32] (columns); kGeneral: PairWeights[32]
constexpr uint32_t kSWref = 32 * 8;                   // byte distance w_alt[i] -> w_ref[i]
constexpr uint32_t kSWhi = kSWtab + 2 * 32 * 8;       // kSingleLds / kMultiLds: uint32 high words of w_alt[32], w_ref[32] (their low words are 0)
constexpr uint32_t kSWhiRef = 32 * 4;                 // byte distance w_alt_hi[i] -> w_ref_hi[i]
constexpr uint32_t kSBins = kSWhi + 2 * 32 * 4;       // kSingleLds: int16 thr[total_bins], uint16 hist[total_bins] (ranks, svt_host_tables.h); kGeneral: LibDesc[n_libs]

struct StreamArgs {
    const uint4* records;        // canonical records; the allocation ends on a 128-byte block boundary, tail zeroed
    const uint64_t* rec_offset;  // n_units + 1
    const svt_unit* units;
    const double* pm;            // 256
    const double* l10;           // n_l10, allocation padded to whole KiB
    const LibDesc* libs;
    const Bin* bins;
    const PairWeights* wtab;     // 32
    uint32_t n_l10;
    uint32_t n_libs;
    uint32_t total_bins;
    uint32_t last_blk;           // index of the last 128-byte block of the records
    uint32_t lds_bins;           // bins staged in LDS (kSingleLds: the whole table)
    uint32_t lds_libs;           // library descriptors staged in LDS
    uint32_t lds_rings;          // byte offset of wave 0's ring (128-byte aligned)
    uint32_t l10_where;          // kL10Shared / kL10Ring / kL10Global
    uint32_t lds_l10;            // kL10Shared: byte offset of the workgroup's copy of the log10 table
    uint32_t l10_lds_entries;    // entries of the table the epilogue finds in LDS (kL10Shared: all; kL10Ring: what one ring stage holds --
                                 // a unit whose read count reaches beyond takes the table through L2; kL10Global: 0)
    uint64_t n_units;
    svt_result* out;
    uint32_t* err;
    // kMultiLds: units grouped by the library window of their sample (svt_unit.libs)
    const uint32_t* perm;        // unit indices, grouped by window, original order inside a group; nullptr = the identity
    const uint2* chunks;         // one per workgroup: {first position in perm, units (<= 256 * R)} -- never crosses a group
    const WgDesc* windows;       // one per workgroup: the libraries / bins it stages
    uint32_t lds_winlibs;        // byte offset of the WinLib descriptors (after the bins)
    uint32_t unit_begin;         // this launch covers units [unit_begin, unit_end) (the pipelined one-shot launches
    uint32_t unit_end;           // one range per uploaded piece; a pass over a resident batch: [0, n_units))
    uint32_t units_per_wg;       // (not the window mode) consecutive units of one workgroup, <= 256 * R: the host cuts a launch into
                                 // EQUAL workgroups that fill whole rounds of the chip's resident workgroups (svtyper_hip.hip: wg_plan)
    uint32_t chunk_begin;        // (library windows) this launch covers the chunks from this one on
    uint32_t result96;           // SVT_FLAG_RESULT96: `out` holds 96-byte records (svt_result96) in the workgroups' own order, tagged with their unit
    uint32_t slot_begin;         // ... the first of them this launch writes (workgroup w of the launch: slot_begin + w * 256 * R)
    uint32_t out_samples;        // svt_batch_result_order: > 1 = the units are sample-major (unit = sample * out_sites + site) and the
    uint32_t out_sites;          // result record of a unit goes to index site * out_samples + sample (site-major); 0 = unit order
    LibDesc lib0;
    GtConsts c;
};

// kMultiLds: one library of the workgroup's window, 32 bytes in LDS
struct WinLib {
    uint32_t kmin;      // (uint32) key_min
    uint32_t nb;        // n_bins == index of the library's sentinel bin
    uint32_t thr_at;    // LDS byte address of this library's thr[0]
    uint32_t hist_at;   // LDS byte address of this library's hist[0]
    double sd2;         // 2 * sd: the small-deletion gate (classic.py:339,383)
    double pad;
};
static_assert(sizeof(WinLib) == 32, "WinLib is read as two 16-byte halves");

// this workgroup's units: `units_per_wg` consecutive ones, or (library windows) a chunk of the permutation that groups the units
// by the libraries of their sample -- at most `chunk_cap` of it
struct WgUnits {
    uint32_t wg_index;   // workgroup of the launch / (library windows) chunk of the batch
    uint32_t wg_base;    // first unit / first position in perm
    uint32_t n_here;     // units of this workgroup
    WgDesc wd;           // library windows: what the workgroup stages
};
template <int MODE>
__device__ __forceinline__ WgUnits wg_units(const StreamArgs& a, const uint32_t chunk_cap = 0xFFFFFFFFu)
{
    WgUnits g;
    g.wg_base = a.unit_begin + blockIdx.x * a.units_per_wg;
    g.wd = WgDesc{};
    g.wg_index = MODE == kMultiLds ? blockIdx.x + a.chunk_begin : blockIdx.x;   // (the launch's chunk range / workgroup)
    if (MODE == kMultiLds) {
        const uint2 ch = a.chunks[g.wg_index];
        g.wg_base = ch.x;
        g.n_here = min(ch.y, chunk_cap);
        g.wd = a.windows[g.wg_index];
    } else {
        g.n_here = min(a.units_per_wg, a.unit_end - g.wg_base);
    }
    return g;
}
// the unit at position `local` of the workgroup (library windows: a.perm == nullptr when the units already come grouped by window)
template <int MODE>
__device__ __forceinline__ uint32_t wg_unit_at(const StreamArgs& a, const uint32_t wg_base, const uint32_t local)
{
    return MODE == kMultiLds && a.perm ? a.perm[wg_base + local] : wg_base + local;
}

// The tables of the layout above, staged by the THREADS threads of the workgroup (no barrier: the sort's barriers follow).
// HI: also the high words at kSWhi.
template <int MODE, uint32_t THREADS, bool HI>
__device__ __forceinline__ void stage_tables(unsigned char* smem, const StreamArgs& a, const WgDesc& wd, const uint32_t tid)
{
    for (uint32_t i = tid; i < 256; i += THREADS) {
        const double p = a.pm[i];
        reinterpret_cast<double*>(smem + kSPm)[i] = p;
        reinterpret_cast<double*>(smem + kSPmHalf)[i] = p * 0.5;
    }
    if (tid < 32) {
        const PairWeights pw = a.wtab[tid];
        if (MODE != kGeneral) {
            reinterpret_cast<double*>(smem + kSWtab)[tid] = pw.w_alt;
            reinterpret_cast<double*>(smem + kSWtab + kSWref)[tid] = pw.w_ref;
            if (HI) {
                reinterpret_cast<uint32_t*>(smem + kSWhi)[tid] = (uint32_t)__double2hiint(pw.w_alt);
                reinterpret_cast<uint32_t*>(smem + kSWhi + kSWhiRef)[tid] = (uint32_t)__double2hiint(pw.w_ref);
            }
        } else {
            reinterpret_cast<PairWeights*>(smem + kSWtab)[tid] = pw;
        }
    }
    if (MODE == kSingleLds) {
        // thr[] and hist[] as two 2-byte arrays (svt_host_tables.h replaced the counts by their ranks, which is
        // all `hist[o - v] <= thr[o]` needs): the random look-ups of a wave spread over every LDS bank
        int16_t* s_thr = reinterpret_cast<int16_t*>(smem + kSBins);
        uint16_t* s_hst = reinterpret_cast<uint16_t*>(smem + kSBins) + a.total_bins;
        for (uint32_t i = tid; i < a.total_bins; i += THREADS) {
            const Bin bn = a.bins[i];
            s_thr[i] = (int16_t)bn.thr;
            s_hst[i] = (uint16_t)bn.hist;
        }
    } else if (MODE == kMultiLds) {
        // the window's bins as thr[bin_cnt], hist[bin_cnt] and one WinLib per library of the window
        int16_t* s_thr = reinterpret_cast<int16_t*>(smem + kSBins);
        uint16_t* s_hst = reinterpret_cast<uint16_t*>(smem + kSBins) + wd.bin_cnt;
        for (uint32_t i = tid; i < wd.bin_cnt; i += THREADS) {
            const Bin bn = a.bins[wd.bin_lo + i];
            s_thr[i] = (int16_t)bn.thr;
            s_hst[i] = (uint16_t)bn.hist;
        }
        if (tid < wd.lib_cnt) {
            const LibDesc L = a.libs[wd.lib_lo + tid];
            WinLib wl;
            wl.kmin = (uint32_t)L.key_min;
            wl.nb = L.n_bins;
            wl.thr_at = kSBins + (L.tab_off - wd.bin_lo) * 2u;
            wl.hist_at = kSBins + (wd.bin_cnt + L.tab_off - wd.bin_lo) * 2u;
            wl.sd2 = L.sd2;
            wl.pad = 0.0;
            reinterpret_cast<WinLib*>(smem + a.lds_winlibs)[tid] = wl;
        }
    } else {
        for (uint32_t i = tid; i < a.n_libs * (uint32_t)(sizeof(LibDesc) / 8); i += THREADS)
            reinterpret_cast<uint64_t*>(smem + kSBins)[i] = reinterpret_cast<const uint64_t*>(a.libs)[i];
    }
    if (a.l10_where == kL10Shared) {
        double* s_l10 = reinterpret_cast<double*>(smem + a.lds_l10);
        for (uint32_t i = tid; i < a.n_l10; i += THREADS) s_l10[i] = a.l10[i];
    }
}

// per-lane constants of the unit for the one-library record consumer
struct StreamCtx {
    uint32_t fmask;    // straddle-bit mask with the small-DEL gate applied (classic.py:339,383)
    uint32_t kmin;     // (uint32) key_min
    uint32_t nb;       // n_bins == index of the sentinel bin
    uint32_t sub2;     // DEL ? var_length + key_min : 0x80000000 (never in range)
    uint32_t hist_at;  // LDS address of hist[0]
    uint32_t wt0, wt1; // LDS address of w_alt[del16] / w_alt[del16 + 8] (p_concordant = 0 / 1)
    uint32_t wh0;      // LDS address of w_alt_hi[del16]
};

// ---- the tile entry of the kernels for small launches: everything a record's look-ups need to know of its unit, by sorted
// position: {first record, records, sub2, flags}
//   sub2   one library: DEL ? var_length + key_min : never in range; windows: DEL ? var_length : never -- the library's key_min
//          is added per record
//   flags  straddle-bit mask with the one-library small-DEL gate applied | DEL ? 16 : 0 | svtype << 8 | svt_unit.flags << 16
constexpr uint32_t kTileFmask = 7u, kTileDel16 = 16u, kTileSvtypeShift = 8u, kTileUflagsShift = 16u;
template <int MODE>
__device__ __forceinline__ uint4 make_tile_entry(const svt_unit& U, const uint32_t beg, const uint32_t cnt, const StreamArgs& a)
{
    const bool is_del = U.svtype == SVT_SVTYPE_DEL;
    const bool small_del = MODE == kSingleLds && is_del && ((double)U.pos_delta < a.lib0.sd2);   // classic.py:339,383
    const uint32_t flags = (small_del ? 0u : kTileFmask) | (is_del ? kTileDel16 : 0u) | ((uint32_t)U.svtype << kTileSvtypeShift) |
                           ((uint32_t)U.flags << kTileUflagsShift);
    const uint32_t sub2 = is_del ? (uint32_t)U.var_length + (MODE == kSingleLds ? (uint32_t)a.lib0.key_min : 0u) : 0x80000000u;
    return make_uint4(beg, cnt, sub2, flags);
}
__device__ __forceinline__ uint32_t tile_svtype(const uint32_t flags) { return (flags >> kTileSvtypeShift) & 0xffu; }
__device__ __forceinline__ uint32_t tile_uflags(const uint32_t flags) { return flags >> kTileUflagsShift; }

// ---- the tail of an epilogue
// where the record goes: the unit's own index, or (svt_batch_result_order) the site-major index of a sample-major unit
__device__ __forceinline__ uint32_t result_destination(const StreamArgs& a, const uint32_t unit)
{
    uint32_t unit_out = unit;
    if (a.out_samples > 1u && unit != kPadUnit) {
        const uint32_t sample = unit / a.out_sites;
        unit_out = (unit - sample * a.out_sites) * a.out_samples + sample;
    }
    return unit_out;
}
// The epilogue of the unit at sorted position p whose five tallies wait in the planes s_tally[5][kBlock] (ref_seq, alt_seq,
// alt_clip, ref_span, alt_span; classic.py:425-513 in unit_epilogue): one unit per lane, the wave's 64 result records leave
// through `ring`.
__device__ __forceinline__ void tally_epilogue(const StreamArgs& a, const unsigned char* smem, const double* s_tally, const uint4* s_tile,
                                               const uint32_t* s_unit, const uint32_t p, unsigned char* ring, const uint32_t lane,
                                               const uint32_t tile_slot)
{
    Acc acc = {s_tally[p], s_tally[kBlock + p], s_tally[2 * kBlock + p], s_tally[3 * kBlock + p], s_tally[4 * kBlock + p], 0.0, 0.0, 0.0};
    const uint32_t unit = s_unit[p], flags = s_tile[p].w;
    const double* lds_l10 = reinterpret_cast<const double*>(smem + a.lds_l10);
    uint4 piece[8];
    unit_epilogue(acc, tile_svtype(flags), tile_uflags(flags), a.c, lds_l10, a.l10, a.l10_where == kL10Shared ? a.l10_lds_entries : 0u, piece);
    const uint32_t unit_out = result_destination(a, unit);
    uint32_t sorted_base = 0xFFFFFFFFu;
    if (a.result96) {
        result96_tag(piece, unit_out);
        sorted_base = tile_slot;
    }
    store_result_records_through_ring(ring, piece, unit_out, lane, reinterpret_cast<unsigned char*>(a.out), a.result96 ? 6u : 8u, sorted_base);
}

}  // namespace svt

#endif  // SVT_WG_PARTS_H

// svt_bam_index.h -- the index of a BAM file, BAI or CSI, as one model (host only; used by svt_reads_handle.h and svt_reads_records.h, parts of svt_reads.cpp).
//
// Both formats say the same thing in two shapes (SAM spec 5.2, CSIv1): per reference a map bin -> chunks over a binning scheme
// of `depth` levels whose leaves span 2^min_shift positions, and something that bounds a fetch from below -- the linear index of a
// BAI (one offset per 16-kbp window), or one `loffset` per bin of a CSI.  A BAI is the scheme (14, 5) and ends at 2^29; a CSI
// names its own (samtools index -c -m: (14, 5) by default, (14, 6) and up for contigs beyond 512 Mbp).  What the reader needs
// of either is here: the bins of a window, the offset no record of the window lies in front of, and the record starts the index
// knows of (the cuts of the library scan).  Nothing outside this header reads `linear`, `loffset` or `bins`.
//
// A CSI is a BGZF file: its members are inflated by the reader's own one-source decoder (svt_inflate.h) and checked against
// their CRC-32 (svt_crc32.h) before a byte is parsed.  Every count and every read is checked against the bytes there are; a
// file that fails a check is refused with a text that names it.  (tests/native/asan_csi_main.cpp runs this header alone under
// AddressSanitizer + UndefinedBehaviorSanitizer.)
#ifndef SVT_BAM_INDEX_H
#define SVT_BAM_INDEX_H

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "svt_crc32.h"
#include "svt_inflate.h"

namespace svt {
namespace bamidx {

enum : int { KIND_NONE = 0, KIND_BAI = 1, KIND_CSI = 2 };      // (svt_bam_index_info's `kind`)

typedef std::pair<uint64_t, uint64_t> Chunk;                   // virtual offsets [first, second)

struct RefIndex {
    std::unordered_map<uint32_t, std::vector<Chunk>> bins;     // without the pseudo-bin
    std::vector<uint64_t> linear;                              // BAI: one offset per 2^14 positions
    std::unordered_map<uint32_t, uint64_t> loffset;            // CSI: per bin
    uint64_t mapped = 0, unmapped = 0;                         // the pseudo-bin's counts (0 without one)
    bool has_counts = false;
};

struct Index {
    int kind = KIND_NONE;
    int min_shift = 14, depth = 5;
    std::vector<RefIndex> refs;
    uint64_t n_no_coor = 0;                                    // the trailing count of reads without coordinates
    bool has_no_coor = false;

    // first bin of level l (0: the root): (8^l - 1) / 7
    static uint32_t level_first(int l) { return (uint32_t)(((1ull << (3 * l)) - 1) / 7); }
    int level_shift(int l) const { return min_shift + 3 * (depth - l); }
    uint32_t pseudo_bin() const { return (uint32_t)(((1ull << (3 * (depth + 1))) - 1) / 7 + 1); }   // 37450 at depth 5
    int64_t max_pos() const { return (int64_t)1 << (min_shift + 3 * depth); }                       // positions below it are covered

    // [beg, end) clipped to what the index covers and to the contig (length <= 0: unknown); false: nothing is left
    bool clip(int64_t& beg, int64_t& end, int64_t contig_length) const
    {
        beg = std::max<int64_t>(beg, 0);
        end = std::min(end, max_pos());
        if (contig_length > 0) end = std::min(end, contig_length);
        return end > beg;
    }

    // the bins that overlap [beg, end), root first; the window is clipped already
    void reg2bins(int64_t beg, int64_t end, std::vector<uint32_t>& out) const
    {
        out.clear();
        if (end <= beg) return;
        --end;
        for (int l = 0; l <= depth; ++l) {
            const int s = level_shift(l);
            const int64_t first = level_first(l);
            for (int64_t k = first + (beg >> s); k <= first + (end >> s); ++k) out.push_back((uint32_t)k);
        }
    }

    // An offset that no record overlapping [beg, ...) on `tid` lies in front of: the filter on chunks (c.second > min_offset).
    // BAI: the linear index's entry of beg's window (the last entry behind its end).  CSI: the rule taken is htslib's -- the
    // loffset of the leaf bin that holds `beg`; where that bin is absent the nearest present one met by stepping to the
    // previous sibling and, from a first sibling, to the parent; 0 when none is present.  Every bin met starts at or below
    // `beg`, and a bin's loffset is the first record that reaches its start, so the value is never behind the window's first record.
    uint64_t min_offset(int32_t tid, int64_t beg) const
    {
        if (tid < 0 || (size_t)tid >= refs.size()) return 0;
        const RefIndex& ri = refs[(size_t)tid];
        if (kind == KIND_BAI) {
            if (ri.linear.empty()) return 0;
            const size_t li = (size_t)(std::max<int64_t>(beg, 0) >> 14);
            return li < ri.linear.size() ? ri.linear[li] : ri.linear.back();
        }
        if (ri.loffset.empty()) return 0;
        beg = std::min(std::max<int64_t>(beg, 0), max_pos() - 1);
        uint32_t bin = level_first(depth) + (uint32_t)(beg >> min_shift);
        for (;;) {
            auto it = ri.loffset.find(bin);
            if (it != ri.loffset.end()) return it->second;
            if (bin == 0) return 0;
            const uint32_t parent = (bin - 1) >> 3, first = (parent << 3) + 1;
            bin = bin > first ? bin - 1 : parent;
        }
    }

    // the merged chunks a fetch of [beg, end) on `tid` walks, in file order; `bins` and `chunks` are the caller's scratch
    void fetch_chunks(int32_t tid, int64_t beg, int64_t end, int64_t contig_length, std::vector<uint32_t>& bins,
                      std::vector<Chunk>& chunks, std::vector<Chunk>& merged) const
    {
        chunks.clear();
        merged.clear();
        if (tid < 0 || (size_t)tid >= refs.size() || !clip(beg, end, contig_length)) return;
        const RefIndex& ri = refs[(size_t)tid];
        const uint64_t min_off = min_offset(tid, beg);
        reg2bins(beg, end, bins);
        for (uint32_t b : bins) {
            auto it = ri.bins.find(b);
            if (it == ri.bins.end()) continue;
            for (const Chunk& c : it->second)
                if (c.second > min_off) chunks.push_back(c);
        }
        if (chunks.empty()) return;
        std::sort(chunks.begin(), chunks.end());
        merged.push_back(chunks[0]);
        for (size_t i = 1; i < chunks.size(); ++i) {
            if (chunks[i].first <= merged.back().second) merged.back().second = std::max(merged.back().second, chunks[i].second);
            else merged.push_back(chunks[i]);
        }
    }

    // The record starts behind `first_record` that the index knows of, ascending and distinct: the cuts of the library scan.
    // BAI: the linear offsets.  CSI (no linear index): the bins' loffsets and the chunks' begins.  The scan proves every cut by
    // walking up to it, so an offset here that is no record start ends in the host scan, never in a wrong answer.
    void record_starts(uint64_t first_record, std::vector<uint64_t>& cuts) const
    {
        cuts.clear();
        for (const RefIndex& ri : refs) {
            if (kind == KIND_BAI) {
                for (uint64_t v : ri.linear)
                    if (v > first_record) cuts.push_back(v);
                continue;
            }
            for (const auto& kv : ri.loffset)
                if (kv.second > first_record) cuts.push_back(kv.second);
            for (const auto& kv : ri.bins)
                for (const Chunk& c : kv.second)
                    if (c.first > first_record) cuts.push_back(c.first);
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    }
};

namespace detail {

inline uint32_t u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t u64(const uint8_t* p) { return (uint64_t)u32(p) | ((uint64_t)u32(p + 4) << 32); }

// a cursor over bytes that answers false instead of reading past them
struct Cursor {
    const uint8_t* p;
    size_t n, at = 0;
    Cursor(const uint8_t* data, size_t size) : p(data), n(size) {}
    size_t left() const { return n - at; }
    bool skip(uint64_t k) { if (k > left()) return false; at += (size_t)k; return true; }
    bool i32(int32_t& v) { if (left() < 4) return false; v = (int32_t)u32(p + at); at += 4; return true; }
    bool w32(uint32_t& v) { if (left() < 4) return false; v = u32(p + at); at += 4; return true; }
    bool w64(uint64_t& v) { if (left() < 8) return false; v = u64(p + at); at += 8; return true; }
};

inline void pseudo_counts(RefIndex& ri, const std::vector<Chunk>& chunks)   // [unmapped beg, end], [n_mapped, n_unmapped]
{
    if (chunks.size() < 2) return;
    ri.mapped = chunks[1].first;
    ri.unmapped = chunks[1].second;
    ri.has_counts = true;
}

}  // namespace detail

// The bytes of a .bai (magic BAI\1).  false: `err` says why.
inline bool load_bai(const uint8_t* data, size_t size, const std::string& name, Index& idx, std::string& err)
{
    idx = Index();
    if (size < 8 || std::memcmp(data, "BAI\1", 4) != 0) { err = name + " is not a BAI index"; return false; }
    auto u32 = [&](size_t o) { return detail::u32(data + o); };
    auto u64 = [&](size_t o) { return detail::u64(data + o); };
    const auto truncated = [&] { err = "truncated BAI: " + name; return false; };
    size_t off = 4;
    const uint32_t nr = u32(off);
    off += 4;
    if ((uint64_t)nr * 8 > size - off) return truncated();      // (a reference takes its two counts at least)
    idx.refs.resize(nr);
    for (uint32_t r = 0; r < nr; ++r) {
        if (off + 4 > size) return truncated();
        const uint32_t n_bin = u32(off);
        off += 4;
        for (uint32_t k = 0; k < n_bin; ++k) {
            if (off + 8 > size) return truncated();
            const uint32_t bin = u32(off), n_chunk = u32(off + 4);
            off += 8;
            if (off + 16ull * n_chunk > size) return truncated();
            std::vector<Chunk> pseudo;
            auto& v = bin != 37450 ? idx.refs[r].bins[bin] : pseudo;
            for (uint32_t c = 0; c < n_chunk; ++c) v.emplace_back(u64(off + 16 * c), u64(off + 16 * c + 8));
            if (bin == 37450) detail::pseudo_counts(idx.refs[r], pseudo);
            off += 16ull * n_chunk;
        }
        if (off + 4 > size) return truncated();
        const uint32_t n_intv = u32(off);
        off += 4;
        if (off + 8ull * n_intv > size) return truncated();
        for (uint32_t k = 0; k < n_intv; ++k) idx.refs[r].linear.push_back(u64(off + 8 * k));
        off += 8ull * n_intv;
    }
    if (off + 8 <= size) { idx.n_no_coor = u64(off); idx.has_no_coor = true; }
    idx.kind = KIND_BAI;
    return true;
}

// The BGZF members of a file side by side, each inflated by svt_inflate.h and checked against its CRC-32.
inline bool inflate_bgzf(const uint8_t* data, size_t size, const std::string& name, std::vector<uint8_t>& out, std::string& err)
{
    out.clear();
    const std::unique_ptr<inf::Scratch> S(new inf::Scratch());
    const std::unique_ptr<crc::Tables> T(new crc::Tables());
    crc::fill_tables(*T);
    crc::Scratch C;
    uint64_t coff = 0;
    while (coff < size) {
        uint64_t src = 0, next = 0;
        uint32_t clen = 0, isize = 0;
        if (!inf::member_at(data, size, coff, src, clen, isize, next)) {
            err = name + ": no BGZF member at offset " + std::to_string(coff) + " (truncated or not a CSI index)";
            return false;
        }
        const size_t at = out.size();
        out.resize(at + isize);
        if (isize) {
            const uint32_t status = inf::inflate_member<inf::HostCtx>(data + src, clen, out.data() + at, isize, *S);
            if (status != inf::INF_OK) {
                err = name + ": the BGZF member at offset " + std::to_string(coff) + " does not inflate (status " + std::to_string(status) + ")";
                return false;
            }
            if (crc::crc_member<crc::HostCtx>(out.data() + at, isize, *T, C) != inf::member_crc(data, src, clen)) {
                err = name + ": the BGZF member at offset " + std::to_string(coff) + " fails its CRC32";
                return false;
            }
        }
        coff = next;
    }
    return true;
}

// The inflated bytes of a .csi (magic CSI\1).  false: `err` says why.
inline bool parse_csi(const uint8_t* data, size_t size, const std::string& name, Index& idx, std::string& err)
{
    idx = Index();
    const auto bad = [&](const char* what) { err = name + ": " + what; return false; };
    if (size < 4 || std::memcmp(data, "CSI\1", 4) != 0) { err = name + " is not a CSI index (wrong magic behind the BGZF layer)"; return false; }
    detail::Cursor c(data, size);
    c.skip(4);
    int32_t min_shift = 0, depth = 0, l_aux = 0, n_ref = 0;
    if (!c.i32(min_shift) || !c.i32(depth) || !c.i32(l_aux)) return bad("truncated CSI header");
    if (min_shift < 0 || depth < 0 || (int64_t)min_shift + 3ll * depth > 62) return bad("CSI min_shift / depth out of range (min_shift + 3 * depth <= 62)");
    if (depth > 10) return bad("CSI depth out of range (bin numbers are 32-bit: depth <= 10)");
    if (l_aux < 0) return bad("negative count in CSI (l_aux)");
    if (!c.skip((uint64_t)l_aux)) return bad("truncated CSI (aux bytes)");
    if (!c.i32(n_ref)) return bad("truncated CSI header");
    if (n_ref < 0) return bad("negative count in CSI (n_ref)");
    if ((uint64_t)n_ref * 4 > c.left()) return bad("truncated CSI (references)");
    idx.min_shift = min_shift;
    idx.depth = depth;
    const uint32_t pseudo = idx.pseudo_bin();
    idx.refs.resize((size_t)n_ref);
    for (int32_t r = 0; r < n_ref; ++r) {
        RefIndex& ri = idx.refs[(size_t)r];
        int32_t n_bin = 0;
        if (!c.i32(n_bin)) return bad("truncated CSI (bins)");
        if (n_bin < 0) return bad("negative count in CSI (n_bin)");
        for (int32_t k = 0; k < n_bin; ++k) {
            uint32_t bin = 0;
            uint64_t loffset = 0;
            int32_t n_chunk = 0;
            if (!c.w32(bin) || !c.w64(loffset) || !c.i32(n_chunk)) return bad("truncated CSI (bins)");
            if (n_chunk < 0) return bad("negative count in CSI (n_chunk)");
            if ((uint64_t)n_chunk * 16 > c.left()) return bad("truncated CSI (chunks)");
            std::vector<Chunk> pseudo_chunks;
            std::vector<Chunk>& v = bin != pseudo ? ri.bins[bin] : pseudo_chunks;
            for (int32_t j = 0; j < n_chunk; ++j) {
                uint64_t a = 0, b = 0;
                c.w64(a);
                c.w64(b);
                v.emplace_back(a, b);
            }
            if (bin == pseudo) detail::pseudo_counts(ri, pseudo_chunks);
            else ri.loffset[bin] = loffset;
        }
    }
    if (c.left() >= 8) { c.w64(idx.n_no_coor); idx.has_no_coor = true; }
    idx.kind = KIND_CSI;
    return true;
}

inline bool load_csi(const uint8_t* data, size_t size, const std::string& name, Index& idx, std::string& err)
{
    std::vector<uint8_t> plain;
    if (!inflate_bgzf(data, size, name, plain, err)) { idx = Index(); return false; }
    return parse_csi(plain.data(), plain.size(), name, idx, err);
}

// An index file's bytes, whatever its name: the magic decides (BAI\1 as it is, a gzip member in front: a CSI).
inline bool load(const uint8_t* data, size_t size, const std::string& name, Index& idx, std::string& err)
{
    if (size >= 2 && data[0] == 31 && data[1] == 139) return load_csi(data, size, name, idx, err);
    if (size >= 4 && std::memcmp(data, "CSI\1", 4) == 0) { idx = Index(); err = name + ": a CSI index that is not BGZF-compressed"; return false; }
    return load_bai(data, size, name, idx, err);
}

}  // namespace bamidx
}  // namespace svt

#endif  // SVT_BAM_INDEX_H

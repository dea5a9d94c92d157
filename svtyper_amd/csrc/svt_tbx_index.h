// svt_tbx_index.h -- the index fold: a line table of the text as written (svt_vcf_lines.h) and the file offsets of the BGZF
// members that hold it -> the uncompressed bytes of a .tbi.  Host code, one pass over the lines; the layout is the published
// one (the tabix format: "TBI\1", n_ref, format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, the names, per contig its
// bins with their chunks and its 16 kb linear index; binning of SAM spec 5.3).  What it writes per contig:
//   chunks    a run of consecutive lines with one bin is one chunk, from the first line's start to the last line's end (the
//             next line's start; the end of the data behind the last line)
//   ioff[w]   for every 16 kb window a line overlaps, the smallest start of such a line; a window no line overlaps takes the
//             value of the next one that has one (the text is sorted: nothing that overlaps a later window starts earlier)
//   bin 37450 the pseudo-bin of SAM spec 5.2: (first start, last end), (lines of the contig, 0)
// The fold of a contig works in a scheme (14, depth) (svt_index_scheme.h): depth 5 is the .tbi's and the .bai's, whose bytes are
// what they always were; with build(..., csi = true) the depth is the smallest that covers the largest end among the body lines
// and the contigs are serialised as CSIv1 (namespace csi below) with the tabix block as aux.
// Byte equality with what htslib's tabix writes for the same file is not claimed.
#ifndef SVT_TBX_INDEX_H
#define SVT_TBX_INDEX_H

#include <map>

#include "svt_index_scheme.h"
#include "svt_vcf_lines.h"

namespace svt {
namespace tbx {

constexpr uint32_t kPseudoBin = 37450;
constexpr uint64_t kUnset = ~0ull;

struct Builder {
    std::vector<uint8_t> out;
    void u32(uint32_t v) { for (int k = 0; k < 4; ++k) out.push_back((uint8_t)(v >> (8 * k))); }
    void u64(uint64_t v) { for (int k = 0; k < 8; ++k) out.push_back((uint8_t)(v >> (8 * k))); }
};

// the fold of one contig, shared with the .bai of svt_bai_index.h (whose records can be unmapped: the pseudo-bin's second count)
struct Contig {
    std::string name;
    std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;
    std::vector<uint64_t> ioff;
    uint64_t lines = 0, unmapped = 0, first = 0, last = 0;
    uint32_t last_bin = ~0u;
    uint32_t depth = idx::kBaiDepth;                // the scheme (14, depth) the bins are numbered in
    // one more record [beg, end) of the contig, behind the others, at virtual offsets [s, e)
    void add(uint64_t beg, uint64_t end, uint64_t s, uint64_t e)
    {
        const uint32_t bin = idx::reg2bin(beg, end, depth);
        if (bin == last_bin) bins[bin].back().second = e;
        else bins[bin].emplace_back(s, e);
        last_bin = bin;
        const uint64_t w1 = (end - 1) >> 14;
        if (ioff.size() <= w1) ioff.resize(w1 + 1, kUnset);
        for (uint64_t w = beg >> 14; w <= w1; ++w) ioff[w] = std::min(ioff[w], s);
        if (!lines++) first = s;
        last = e;
    }
    // a window no record overlaps takes the value of the next one that has one
    void backfill()
    {
        for (uint64_t w = ioff.size(); w-- > 1;)
            if (ioff[w - 1] == kUnset) ioff[w - 1] = ioff[w];
    }
    // n_bin, the bins, the pseudo-bin, n_intv, the linear index; a contig without records: n_bin = 0, n_intv = 0
    void write(Builder& b)
    {
        if (!lines) {
            b.u32(0); b.u32(0);
            return;
        }
        b.u32((uint32_t)bins.size() + 1);
        for (const auto& bin : bins) {
            b.u32(bin.first);
            b.u32((uint32_t)bin.second.size());
            for (const auto& chunk : bin.second) { b.u64(chunk.first); b.u64(chunk.second); }
        }
        b.u32(kPseudoBin); b.u32(2);
        b.u64(first); b.u64(last); b.u64(lines - unmapped); b.u64(unmapped);
        backfill();
        b.u32((uint32_t)ioff.size());
        for (uint64_t v : ioff) b.u64(v);
    }
};

}  // namespace tbx

// ---- CSIv1 (the published layout): "CSI\1", min_shift, depth, l_aux, aux, n_ref; per reference n_bin and, bins in rising order,
// bin, loffset, n_chunk, the chunks; the pseudo-bin (8^(depth+1) - 1) / 7 + 1 with loffset 0 and (first start, last end),
// (mapped, unmapped); n_bin = 0 for a reference without records; the 64-bit n_no_coor at the end.  ONE serialiser for what the
// host fold leaves (tbx::Contig) and for what the device fold brings down (svt_entry_bam_index.h): the runs -- a run of
// consecutive records with one bin is one chunk -- in stable order by key = tid << 32 | bin, the loffset of every group head
// (a run whose key differs from the one in front), and a row per reference.
namespace csi {

using idx::RefRow;
using idx::Run;

// loff[r] is read for group heads only
inline void serialise(tbx::Builder& b, uint32_t depth, const std::vector<uint8_t>& aux, uint64_t n_ref, const Run* runs, uint64_t n_runs, const uint64_t* loff,
                      const RefRow* rows, uint64_t no_coor)
{
    b.out.assign({'C', 'S', 'I', 1});
    b.u32(idx::kMinShift); b.u32(depth); b.u32((uint32_t)aux.size());
    b.out.insert(b.out.end(), aux.begin(), aux.end());
    b.u32((uint32_t)n_ref);
    uint64_t r = 0;
    for (uint64_t tid = 0; tid < n_ref; ++tid) {
        uint64_t stop = r, n_bin = 0;
        for (; stop < n_runs && runs[stop].key >> 32 == tid; ++stop)
            if (stop == r || runs[stop].key != runs[stop - 1].key) ++n_bin;
        if (rows[tid].mapped + rows[tid].unmapped == 0) {
            b.u32(0);
            r = stop;
            continue;
        }
        b.u32((uint32_t)n_bin + 1);
        while (r < stop) {
            uint64_t g = r + 1;
            while (g < stop && runs[g].key == runs[r].key) ++g;
            b.u32((uint32_t)runs[r].key); b.u64(loff[r]); b.u32((uint32_t)(g - r));
            for (; r < g; ++r) { b.u64(runs[r].s); b.u64(runs[r].e); }
        }
        b.u32(idx::pseudo_bin(depth)); b.u64(0); b.u32(2);
        b.u64(rows[tid].first); b.u64(rows[tid].last); b.u64(rows[tid].mapped); b.u64(rows[tid].unmapped);
    }
    b.u64(no_coor);
}

// the folded contigs as runs, loffsets and rows.  The loffset of a bin -- the start of the first record of the contig, in file
// order, that ends behind the bin's first position -- is the back-filled linear index at the bin's first window: the records
// are sorted by beg, so no record in front of that one overlaps the window or anything behind it.
inline void write(tbx::Builder& b, uint32_t depth, const std::vector<uint8_t>& aux, std::vector<tbx::Contig>& contigs, uint64_t no_coor)
{
    std::vector<Run> runs;
    std::vector<uint64_t> loff;
    std::vector<RefRow> rows(contigs.size());
    for (size_t tid = 0; tid < contigs.size(); ++tid) {
        tbx::Contig& c = contigs[tid];
        rows[tid] = RefRow{c.first, c.last, c.lines - c.unmapped, c.unmapped};
        c.backfill();
        for (const auto& bin : c.bins) {
            const uint64_t w = idx::bin_start(bin.first, depth) >> idx::kMinShift;
            for (const auto& chunk : bin.second) {
                runs.push_back(Run{(uint64_t)tid << 32 | bin.first, chunk.first, chunk.second});
                loff.push_back(w < c.ioff.size() ? c.ioff[w] : c.first);
            }
        }
    }
    serialise(b, depth, aux, contigs.size(), runs.data(), runs.size(), loff.data(), rows.data(), no_coor);
}

}  // namespace csi

namespace tbx {

// svt_tbx_build (include/svtyper_reads.h) without its argument checks: 0 and the bytes in `out`, or the 1-based number of the line
// the index cannot hold and why
inline uint64_t build(const uint8_t* text, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n, uint64_t len, const uint64_t* member_off,
                      uint64_t n_members, uint32_t payload, std::vector<uint8_t>& out, uint32_t& bad_kind, bool csi = false)
{
    // the virtual offset of text position x: a position behind the last payload is the end of the members
    auto voff = [&](uint64_t x) {
        const uint64_t k = x / payload;
        return k >= n_members ? member_off[n_members] << 16 : member_off[k] << 16 | (x - k * payload);
    };
    (void)len;
    std::vector<Contig> contigs;
    std::unordered_map<std::string, uint32_t> tid_of;
    Contig* cur = nullptr;
    std::string name;
    uint64_t last_beg = 0;
    uint32_t depth = idx::kBaiDepth;
    if (csi) {                                      // the smallest scheme that covers the largest end among the body lines
        uint64_t max_end = 0;
        for (uint64_t i = header_lines(lines, n); i < n; ++i)
            if (!(lines[i].flags & (SVT_TBX_META | SVT_TBX_BAD))) max_end = std::max<uint64_t>(max_end, std::max<uint64_t>(lines[i].end, (uint64_t)lines[i].beg + 1));
        depth = std::min(idx::depth_for(max_end), idx::kMaxDepth);
    }
    for (uint64_t i = header_lines(lines, n); i < n; ++i) {
        const svt_tbx_line& l = lines[i];
        if (l.flags & (SVT_TBX_META | SVT_TBX_BAD)) { bad_kind = SVT_TBX_NOT_DATA; return i + 1; }
        if (csi ? l.end == kSaturated || l.end > idx::scheme_end(depth) : (l.flags & SVT_TBX_RANGE) != 0) { bad_kind = SVT_TBX_BEYOND; return i + 1; }
        const uint8_t* p = text + (src_off ? src_off[i] : l.off);
        const bool same = cur && cur->name.size() == l.chrom_len && std::memcmp(cur->name.data(), p, l.chrom_len) == 0;
        if (!same) {
            name.assign((const char*)p, l.chrom_len);
            if (!tid_of.emplace(name, (uint32_t)contigs.size()).second) { bad_kind = SVT_TBX_CONTIG_AGAIN; return i + 1; }
            contigs.emplace_back();
            cur = &contigs.back();
            cur->name = name;
            cur->depth = depth;
        } else if (l.beg < last_beg) { bad_kind = SVT_TBX_POS_BACK; return i + 1; }
        last_beg = l.beg;
        const uint64_t beg = l.beg, end = std::max<uint64_t>(l.end, beg + 1);      // (an empty REF still takes its base)
        const uint64_t s = voff(l.off), e = voff(l.off + l.len);
        cur->add(beg, end, s, e);
    }
    Builder b, names;                               // the tabix block: format 2 (VCF), col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, the names
    names.u32(2); names.u32(1); names.u32(2); names.u32(0); names.u32('#'); names.u32(0);
    uint64_t l_nm = 0;
    for (const Contig& c : contigs) l_nm += c.name.size() + 1;
    names.u32((uint32_t)l_nm);
    for (const Contig& c : contigs) {
        names.out.insert(names.out.end(), c.name.begin(), c.name.end());
        names.out.push_back(0);
    }
    if (csi) {
        csi::write(b, depth, names.out, contigs, 0);
        out.swap(b.out);
        return 0;
    }
    b.out.assign({'T', 'B', 'I', 1});
    b.u32((uint32_t)contigs.size());
    b.out.insert(b.out.end(), names.out.begin(), names.out.end());
    for (Contig& c : contigs) c.write(b);
    out.swap(b.out);
    return 0;
}

}  // namespace tbx
}  // namespace svt

#endif  // SVT_TBX_INDEX_H

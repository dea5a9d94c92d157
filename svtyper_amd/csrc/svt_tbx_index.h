// svt_tbx_index.h -- the index fold: a line table of the text as written (svt_vcf_lines.h) and the file offsets of the BGZF
// members that hold it -> the uncompressed bytes of a .tbi.  Host code, one pass over the lines; the layout is the published
// one (the tabix format: "TBI\1", n_ref, format 2, col_seq 1, col_beg 2, col_end 0, meta '#', skip 0, the names, per contig its
// bins with their chunks and its 16 kb linear index; binning of SAM spec 5.3).  What it writes per contig:
//   chunks    a run of consecutive lines with one bin is one chunk, from the first line's start to the last line's end (the
//             next line's start; the end of the data behind the last line)
//   ioff[w]   for every 16 kb window a line overlaps, the smallest start of such a line; a window no line overlaps takes the
//             value of the next one that has one (the text is sorted: nothing that overlaps a later window starts earlier)
//   bin 37450 the pseudo-bin of SAM spec 5.2: (first start, last end), (lines of the contig, 0)
// Byte equality with what htslib's tabix writes for the same file is not claimed.
#ifndef SVT_TBX_INDEX_H
#define SVT_TBX_INDEX_H

#include <map>

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
    // one more record [beg, end) of the contig, behind the others, at virtual offsets [s, e)
    void add(uint64_t beg, uint64_t end, uint64_t s, uint64_t e)
    {
        const uint32_t bin = reg2bin(beg, end);
        if (bin == last_bin) bins[bin].back().second = e;
        else bins[bin].emplace_back(s, e);
        last_bin = bin;
        const uint64_t w1 = (end - 1) >> 14;
        if (ioff.size() <= w1) ioff.resize(w1 + 1, kUnset);
        for (uint64_t w = beg >> 14; w <= w1; ++w) ioff[w] = std::min(ioff[w], s);
        if (!lines++) first = s;
        last = e;
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
        for (uint64_t w = ioff.size(); w-- > 1;)
            if (ioff[w - 1] == kUnset) ioff[w - 1] = ioff[w];
        b.u32((uint32_t)ioff.size());
        for (uint64_t v : ioff) b.u64(v);
    }
};

// svt_tbx_build (include/svtyper_reads.h) without its argument checks: 0 and the bytes in `out`, or the 1-based number of the line
// the index cannot hold and why
inline uint64_t build(const uint8_t* text, const uint64_t* src_off, const svt_tbx_line* lines, uint64_t n, uint64_t len, const uint64_t* member_off,
                      uint64_t n_members, uint32_t payload, std::vector<uint8_t>& out, uint32_t& bad_kind)
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
    for (uint64_t i = header_lines(lines, n); i < n; ++i) {
        const svt_tbx_line& l = lines[i];
        if (l.flags & (SVT_TBX_META | SVT_TBX_BAD)) { bad_kind = SVT_TBX_NOT_DATA; return i + 1; }
        if (l.flags & SVT_TBX_RANGE) { bad_kind = SVT_TBX_BEYOND; return i + 1; }
        const uint8_t* p = text + (src_off ? src_off[i] : l.off);
        const bool same = cur && cur->name.size() == l.chrom_len && std::memcmp(cur->name.data(), p, l.chrom_len) == 0;
        if (!same) {
            name.assign((const char*)p, l.chrom_len);
            if (!tid_of.emplace(name, (uint32_t)contigs.size()).second) { bad_kind = SVT_TBX_CONTIG_AGAIN; return i + 1; }
            contigs.emplace_back();
            cur = &contigs.back();
            cur->name = name;
        } else if (l.beg < last_beg) { bad_kind = SVT_TBX_POS_BACK; return i + 1; }
        last_beg = l.beg;
        const uint64_t beg = l.beg, end = std::max<uint64_t>(l.end, beg + 1);      // (an empty REF still takes its base)
        const uint64_t s = voff(l.off), e = voff(l.off + l.len);
        cur->add(beg, end, s, e);
    }
    Builder b;
    b.out.assign({'T', 'B', 'I', 1});
    b.u32((uint32_t)contigs.size());
    b.u32(2); b.u32(1); b.u32(2); b.u32(0); b.u32('#'); b.u32(0);
    uint64_t l_nm = 0;
    for (const Contig& c : contigs) l_nm += c.name.size() + 1;
    b.u32((uint32_t)l_nm);
    for (const Contig& c : contigs) {
        b.out.insert(b.out.end(), c.name.begin(), c.name.end());
        b.out.push_back(0);
    }
    for (Contig& c : contigs) c.write(b);
    out.swap(b.out);
    return 0;
}

}  // namespace tbx
}  // namespace svt

#endif  // SVT_TBX_INDEX_H

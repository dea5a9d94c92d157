// svt_vcf_lines.h -- VCF text as lines: the per-line rule of the tabix VCF preset, the line table, the order --sort writes and
// the gather (include/svtyper_reads.h: svt_tbx_line).
//
// ONE piece of source for both places that run the rule, as svt_deflate.h and svt_inflate.h are: parse_line is compiled for the
// host (svt_vcf_lines_host, any C++17 compiler: this is where it is proven against the restatement of tests/tbxcases.py and
// sanitised) and for the device (svt_vcf_lines_kernel.h, one lane per line).  It reads the first eight columns of a line and
// nothing behind them, every byte checked against the line's length; no std::, no allocation.  The host twins of the kernels
// (lines_host, gather_host) and what is host code on both routes (sort_order: contig names to ranks, the stable order) stand
// below it.
#ifndef SVT_VCF_LINES_H
#define SVT_VCF_LINES_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_geometry_math.h"
#include "svt_index_scheme.h"

namespace svt {
namespace tbx {

constexpr uint64_t kTile = 4096;                // bytes of text whose newlines one wavefront counts (64 lanes x 16 bytes x 4)
constexpr uint64_t kTbiEnd = 1ull << 29;        // a TBI index addresses [0, 2^29)
constexpr uint32_t kSaturated = 0xFFFFFFFFu;

SVT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// the line p[0, len) (its newline included where it has one) -> beg, end, chrom_len and flags of r; off and len are the caller's
SVT_HD void parse_line(const uint8_t* p, uint64_t len, svt_tbx_line& r)
{
    r.beg = r.end = r.chrom_len = 0;
    r.flags = 0;
    const uint64_t n = len && p[len - 1] == '\n' ? len - 1 : len;
    if (n && p[0] == '#') {
        r.flags = SVT_TBX_META;
        return;
    }
    r.flags = SVT_TBX_BAD;                      // until the eighth column is reached
    uint64_t at = 0, pos = 0, ref_len = 0, chrom_len = 0, info = 0, info_end = 0;
    for (uint32_t col = 0; col < 8; ++col) {
        uint64_t e = at;
        while (e < n && p[e] != '\t') ++e;
        if (col < 7 && e == n) return;          // fewer than eight columns (an empty line has none)
        if (col == 0) chrom_len = e - at;
        else if (col == 1) {
            if (e == at || e - at > 10) return;
            for (uint64_t i = at; i < e; ++i) {
                if (!is_digit(p[i])) return;
                pos = pos * 10 + (p[i] - '0');
            }
            if (pos >= (1ull << 31)) return;
        } else if (col == 3) ref_len = e - at;
        else if (col == 7) {
            info = at;
            info_end = e;
        }
        at = e + 1;
    }
    const uint64_t beg = pos ? pos - 1 : 0;
    uint64_t end = beg + ref_len;
    for (uint64_t i = info; i + 5 <= info_end; ++i) {
        if (i != info && p[i - 1] != ';') continue;
        if (p[i] != 'E' || p[i + 1] != 'N' || p[i + 2] != 'D' || p[i + 3] != '=' || !is_digit(p[i + 4])) continue;
        uint64_t v = 0, digits = 0;                 // the first such key decides
        for (uint64_t k = i + 4; k < info_end && is_digit(p[k]); ++k, ++digits)
            if (digits < 11) v = v * 10 + (p[k] - '0');
        if (digits <= 10 && v > beg) end = v;
        break;
    }
    r.flags = end > kTbiEnd ? SVT_TBX_RANGE : 0;
    r.beg = (uint32_t)beg;
    r.end = end > kSaturated ? kSaturated : (uint32_t)end;
    r.chrom_len = chrom_len > kSaturated ? kSaturated : (uint32_t)chrom_len;
}

// the bin of [beg, end) (SAM spec 5.3: 14-bit leaves, five levels)
SVT_HD uint32_t reg2bin(uint64_t beg, uint64_t end) { return idx::reg2bin(beg, end, idx::kBaiDepth); }

}  // namespace tbx
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace svt {
namespace tbx {

inline uint64_t count_lines(const uint8_t* text, uint64_t len)
{
    uint64_t n = 0, at = 0;
    while (at < len) {
        const void* nl = std::memchr(text + at, '\n', len - at);
        ++n;
        if (!nl) break;
        at = (uint64_t)((const uint8_t*)nl - text) + 1;
    }
    return n;
}

// the line table of text[0, len) into lines[0, count_lines(text, len))
inline void lines_host(const uint8_t* text, uint64_t len, svt_tbx_line* lines)
{
    uint64_t i = 0, at = 0;
    while (at < len) {
        const void* nl = std::memchr(text + at, '\n', len - at);
        const uint64_t end = nl ? (uint64_t)((const uint8_t*)nl - text) + 1 : len;
        lines[i].off = at;
        lines[i].len = end - at;
        parse_line(text + at, end - at, lines[i]);
        ++i;
        at = end;
    }
}

// what the gather may touch: every line inside the text, every entry of perm a line, the lines' lengths summing to out_len;
// dst_off[j]: where line j of the output begins
inline const char* gather_plan(uint64_t len, const svt_tbx_line* lines, uint64_t n, const uint64_t* perm, uint64_t n_perm, uint64_t out_len,
                               std::vector<uint64_t>& dst_off)
{
    dst_off.resize(n_perm);
    uint64_t at = 0;
    for (uint64_t j = 0; j < n_perm; ++j) {
        if (perm[j] >= n) return "svt_vcf_gather: an entry of perm is no line";
        const svt_tbx_line& l = lines[perm[j]];
        if (l.off > len || l.len > len - l.off) return "svt_vcf_gather: a line lies outside the text";
        if (l.len > out_len - at) return "svt_vcf_gather: out_len is below the lines' lengths";
        dst_off[j] = at;
        at += l.len;
    }
    return at == out_len ? nullptr : "svt_vcf_gather: out_len is above the lines' lengths";
}

inline void gather_host(const uint8_t* text, const svt_tbx_line* lines, const uint64_t* perm, uint64_t n_perm, const uint64_t* dst_off, uint8_t* out)
{
    for (uint64_t j = 0; j < n_perm; ++j)
        if (lines[perm[j]].len) std::memcpy(out + dst_off[j], text + lines[perm[j]].off, lines[perm[j]].len);
}

// the lines in front of the first line that is no '#' line
inline uint64_t header_lines(const svt_tbx_line* lines, uint64_t n)
{
    uint64_t h = 0;
    while (h < n && (lines[h].flags & SVT_TBX_META)) ++h;
    return h;
}

// the name a header line declares as ##contig=<ID=name...>: ID at the start of the brackets or behind a comma
inline bool contig_id(const uint8_t* p, uint64_t n, std::string& name)
{
    static const char kLead[] = "##contig=<";
    const uint64_t lead = sizeof(kLead) - 1;
    if (n < lead || std::memcmp(p, kLead, lead) != 0) return false;
    for (uint64_t i = lead; i + 3 <= n; ++i) {
        if ((i != lead && p[i - 1] != ',') || p[i] != 'I' || p[i + 1] != 'D' || p[i + 2] != '=') continue;
        uint64_t e = i + 3;
        while (e < n && p[e] != ',' && p[e] != '>' && p[e] != '\n') ++e;
        name.assign((const char*)p + i + 3, e - (i + 3));
        return true;
    }
    return false;
}

// svt_vcf_sort_order (include/svtyper_reads.h): returns the 1-based number of a body line that is no data line, 0 with perm filled
inline uint64_t sort_order(const uint8_t* text, const svt_tbx_line* lines, uint64_t n, uint64_t* perm)
{
    const uint64_t h = header_lines(lines, n);
    std::unordered_map<std::string, uint32_t> rank;
    std::string name;
    for (uint64_t i = 0; i < h; ++i) {
        perm[i] = i;
        if (contig_id(text + lines[i].off, lines[i].len, name)) rank.emplace(name, (uint32_t)rank.size());
    }
    std::vector<std::pair<uint64_t, uint64_t>> keys(n - h);
    for (uint64_t i = h; i < n; ++i) {
        const svt_tbx_line& l = lines[i];
        if (l.flags & (SVT_TBX_META | SVT_TBX_BAD)) return i + 1;
        const uint8_t* p = text + l.off;
        name.assign((const char*)p, l.chrom_len);
        const uint32_t r = rank.emplace(name, (uint32_t)rank.size()).first->second;
        uint64_t pos = 0;                           // (POS itself: POS 0 and POS 1 share a beg)
        for (uint64_t k = (uint64_t)l.chrom_len + 1; k < l.len && is_digit(p[k]); ++k) pos = pos * 10 + (p[k] - '0');
        keys[i - h] = {(uint64_t)r << 32 | pos, i};
    }
    std::sort(keys.begin(), keys.end());            // (the line number is the last key: stable)
    for (uint64_t i = h; i < n; ++i) perm[i] = keys[i - h].second;
    return 0;
}

}  // namespace tbx
}  // namespace svt
#endif  // SVT_VCF_LINES_H

// svt_vcf_paste.h -- per-sample VCFs joined by line number, with AF and NSAMP: the per-line rule, the host twin of the kernels and
// the builder of an output line's first columns (include/svtyper_reads.h: svt_paste_line).
//
// ONE piece of source for both places that run the rule, as svt_bcf.h and svt_vcf_lines.h are: scan_line and measure_input are
// compiled for the host (measure_host, any C++17 compiler: this is where they are proven against goldens made from the reference's
// scripts/vcf_paste.py and scripts/vcf_allele_freq.py, and sanitised) and for the device (svt_vcf_paste_kernel.h, one lane per
// input).  Every load is checked against the line's length; no std::, no allocation, no array indexed by data.
//
// The character classes and Python's float(), int() and '%0.2f' are svt_vcf_cohort_line.h's, shared with the rules over cohort lines.
//
// What the scripts do with one input's line: right-strip it, split it at the first nine tabs, read column 6 as a float, take
// column 9 of the first input as FORMAT, and append whatever stands behind the ninth tab (the "sample part", tabs inside it
// included).  vcf_allele_freq.py then reads the first ':'-subfield of every column of every part as a GT.
//
// The envelope.  A QUAL is read by bcf::double_exact (one exactly rounded IEEE operation); a GT is decimal allele indices of at
// most three digits joined by one kind of separator, at most kMaxPloidy of them, none above the ALT count, which is at most
// kMaxAlt; a part has at most kMaxPartColumns columns; a line has at least nine columns.  Anything else marks the line
// (SVT_PASTE_SLOW_*): nothing is guessed, the host's slow_line decides it in plain C++ with strtod and either writes the
// reference's bytes or names the error.
#ifndef SVT_VCF_PASTE_H
#define SVT_VCF_PASTE_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"
#include "svt_vcf_cohort_line.h"

namespace svt {
namespace paste {

constexpr uint32_t kMaxAlt = 7, kMaxPloidy = 8, kMaxPartColumns = 64, kMaxAlleleDigits = 3;
constexpr uint32_t kNoInput = 0xFFFFFFFFu, kNoField = 3;
constexpr uint32_t kSlowMask = SVT_PASTE_SLOW_QUAL | SVT_PASTE_SLOW_COLUMNS | SVT_PASTE_SLOW_GT | SVT_PASTE_SLOW_ALLELE | SVT_PASTE_SLOW_ALT;

using cohort::is_digit;
using cohort::is_space;
using cohort::kMaxLine;

// where the columns of one right-stripped line lie
struct Scan {
    uint32_t n;                                     // the line's length without its trailing blanks
    uint32_t cols;                                  // 1 .. 9 columns, 10: a tenth column and maybe more behind it
    uint32_t chrom_end, pos_b, pos_end, id_b, id_end;
    uint32_t alt_b, alt_e, qual_b, qual_e, fmt_b, fmt_e;
    uint32_t part_b, part_len;                      // behind the ninth tab: what the reference appends for this input (0: nothing)
};

SVT_HD void scan_line(const uint8_t* p, uint64_t len, Scan& s)
{
    uint32_t n = len > kMaxLine ? kMaxLine : (uint32_t)len;
    while (n && is_space(p[n - 1])) --n;
    s.n = n;
    s.cols = 0;
    s.chrom_end = s.pos_b = s.pos_end = s.id_b = s.id_end = n;
    s.alt_b = s.alt_e = s.qual_b = s.qual_e = s.fmt_b = s.fmt_e = n;
    s.part_b = n;
    s.part_len = 0;
    uint32_t at = 0;
    bool more = true;
    while (more && s.cols < 9) {
        uint32_t e = at;
        while (e < n && p[e] != '\t') ++e;
        if (s.cols == 0) s.chrom_end = e;
        else if (s.cols == 1) { s.pos_b = at; s.pos_end = e; }
        else if (s.cols == 2) { s.id_b = at; s.id_end = e; }
        else if (s.cols == 4) { s.alt_b = at; s.alt_e = e; }
        else if (s.cols == 5) { s.qual_b = at; s.qual_e = e; }
        else if (s.cols == 8) { s.fmt_b = at; s.fmt_e = e; }
        ++s.cols;
        if (e == n) more = false;
        else at = e + 1;
    }
    if (more) {                                     // (behind a tab and right-stripped: at least one byte)
        s.cols = 10;
        s.part_b = at;
        s.part_len = n - at;
    }
}

// the ALT column's alleles: its commas and one
SVT_HD uint32_t count_alts(const uint8_t* p, const Scan& s)
{
    uint32_t k = 1;
    for (uint32_t i = s.alt_b; i < s.alt_e; ++i) k += p[i] == ',';
    return k;
}

// one allele of a GT into its 16-bit field; an index above the ALT count (or above what the fields hold: such a line is marked for
// its ALTs already) is the mark
SVT_HD uint32_t count_allele(uint32_t value, uint32_t n_alt, uint64_t& lo, uint64_t& hi)
{
    if (value > n_alt || value > kMaxAlt) return SVT_PASTE_SLOW_ALLELE;
    if (value < 4) lo += 1ull << (16 * value);
    else hi += 1ull << (16 * (value - 4));
    return 0;
}

// The GTs of one sample part p[b, e): allele a adds one to the 16-bit field a of lo (a < 4) or hi (a - 4): at most
// kMaxPartColumns * kMaxPloidy per field, so none overflows.  Returns the SVT_PASTE_SLOW_* of what is outside the envelope.
SVT_HD uint32_t tally_part(const uint8_t* p, uint32_t b, uint32_t e, uint32_t n_alt, uint64_t& lo, uint64_t& hi, uint32_t& nonref)
{
    uint32_t columns = 0;
    for (uint32_t at = b; at <= e;) {
        if (++columns > kMaxPartColumns) return SVT_PASTE_SLOW_GT;
        uint64_t t_lo = 0, t_hi = 0;                // this GT's alleles: they count only where the token has no '.'
        uint32_t sum = 0, ploidy = 0, digits = 0, value = 0, bad = 0;
        uint8_t sep = 0;
        bool dot = false;
        uint32_t i = at;
        for (; i < e && p[i] != '\t' && p[i] != ':'; ++i) {
            const uint8_t c = p[i];
            if (c == '.') dot = true;
            else if (is_digit(c)) {
                value = value * 10 + (c - '0');
                if (++digits > kMaxAlleleDigits) bad |= SVT_PASTE_SLOW_GT;
            } else if ((c == '/' || c == '|') && digits && (!sep || sep == c)) {
                sep = c;
                bad |= count_allele(value, n_alt, t_lo, t_hi);
                sum += value;
                ++ploidy;
                digits = value = 0;
            } else bad |= SVT_PASTE_SLOW_GT;
        }
        if (!digits) bad |= SVT_PASTE_SLOW_GT;      // an empty token, or one that ends in a separator
        else {
            bad |= count_allele(value, n_alt, t_lo, t_hi);
            sum += value;
            ++ploidy;
        }
        if (ploidy > kMaxPloidy) bad |= SVT_PASTE_SLOW_GT;
        if (!dot) {
            if (bad) return bad;
            lo += t_lo;
            hi += t_hi;
            nonref += sum > 0;
        }
        while (i < e && p[i] != '\t') ++i;          // the other subfields
        at = i + 1;
    }
    return 0;
}

// columns CHROM, POS, ID of line a against line b: the first that differs, kNoField where none does
SVT_HD uint32_t first_unequal(const uint8_t* a, const Scan& sa, const uint8_t* b, const Scan& sb)
{
    for (uint32_t f = 0; f < 3; ++f) {
        const uint32_t ab = f == 0 ? 0 : f == 1 ? sa.pos_b : sa.id_b, ae = f == 0 ? sa.chrom_end : f == 1 ? sa.pos_end : sa.id_end;
        const uint32_t bb = f == 0 ? 0 : f == 1 ? sb.pos_b : sb.id_b, be = f == 0 ? sb.chrom_end : f == 1 ? sb.pos_end : sb.id_end;
        if (sa.cols <= f || sb.cols <= f || ae - ab != be - bb) return f;
        for (uint32_t i = 0; i < ae - ab; ++i)
            if (a[ab + i] != b[bb + i]) return f;
    }
    return kNoField;
}

// what the master's line gives: its QUAL, its ALT count and its marks
struct Master {
    Scan s;
    double qual;
    uint32_t n_alt, slow;
};

SVT_HD void measure_master(const uint8_t* p, uint64_t len, uint32_t flags, Master& m)
{
    scan_line(p, len, m.s);
    m.qual = 0.0;
    m.slow = 0;
    m.n_alt = 1;
    if (len > kMaxLine || m.s.cols < ((flags & SVT_PASTE_AFREQ) ? 8u : 6u)) m.slow |= SVT_PASTE_SLOW_COLUMNS;
    else if (bcf::double_exact(p, m.s.qual_b, m.s.qual_e, m.qual)) m.slow |= SVT_PASTE_SLOW_QUAL;
    if (m.s.cols >= 5) m.n_alt = count_alts(p, m.s);
    if ((flags & SVT_PASTE_AFREQ) && m.n_alt > kMaxAlt) m.slow |= SVT_PASTE_SLOW_ALT;
}

// what one input's line gives
struct Input {
    double qual;
    uint64_t lo, hi;                                // allele counts, 16 bits each (tally_part)
    uint32_t nonref, slow, unequal;                 // unequal: first_unequal against the master (flags & SVT_PASTE_SAFE), else kNoField
    uint32_t part_b, part_len;
};

SVT_HD void measure_input(const uint8_t* p, uint64_t len, const uint8_t* master, const Master& m, uint32_t flags, Input& r)
{
    Scan s;
    scan_line(p, len, s);
    r.qual = 0.0;
    r.lo = r.hi = 0;
    r.nonref = r.slow = 0;
    r.unequal = kNoField;
    r.part_b = s.part_b;
    r.part_len = s.part_len;
    if (len > kMaxLine || s.cols < 9) r.slow |= SVT_PASTE_SLOW_COLUMNS;
    else if (bcf::double_exact(p, s.qual_b, s.qual_e, r.qual)) r.slow |= SVT_PASTE_SLOW_QUAL;
    if ((flags & SVT_PASTE_AFREQ) && s.part_len) r.slow |= tally_part(p, s.part_b, s.part_b + s.part_len, m.n_alt, r.lo, r.hi, r.nonref);
    if (flags & SVT_PASTE_SAFE) r.unequal = first_unequal(p, s, master, m.s);
}

// where one input's part lies in its line and goes in the output line, behind the line's first columns (len 0: no part, nothing goes)
struct Place {
    uint32_t src, len, dst;
};

}  // namespace paste
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace svt {
namespace paste {

// one block of lines: the master's n_lines lines and every input's, side by side in one text under one line table
struct Block {
    const uint8_t* text = nullptr;
    uint64_t len = 0;
    const svt_tbx_line* lines = nullptr;
    uint64_t n_table = 0;
    const uint64_t* first_line = nullptr;          // [n_inputs + 1]: file f's line j is lines[first_line[f] + j]; file 0 is the master
    uint32_t n_inputs = 0;
    uint64_t n_lines = 0;
    uint32_t flags = 0;
    std::vector<std::pair<std::string, bool>> info; // --afreq: the header's INFO ids in its order, and whether the Type is Flag
    const uint8_t* line(uint32_t file, uint64_t j) const { return text + lines[first_line[file] + j].off; }
    uint64_t line_len(uint32_t file, uint64_t j) const { return lines[first_line[file] + j].len; }
};

using cohort::fixed2;
using cohort::parse_info_table;
using cohort::py_float;
using cohort::py_int_text;

inline const char* check_block(const Block& b)
{
    if (!b.n_inputs) return "svt_vcf_paste: no input";
    for (uint32_t f = 0; f <= b.n_inputs; ++f)
        if (b.first_line[f] > b.n_table || b.n_lines > b.n_table - b.first_line[f]) return "svt_vcf_paste: a file's lines lie outside the line table";
    if (b.n_lines > 0xFFFFFFFFull / ((uint64_t)b.n_inputs + 1)) return "svt_vcf_paste: a block holds less than 2^32 lines";
    return nullptr;
}

// the arguments of both entry points as a Block, `info` cleared; or what is wrong with them
inline const char* take_arguments(const uint8_t* text, uint64_t len, const uint64_t* first_line, uint32_t n_inputs, uint64_t n_lines, uint32_t flags,
                                  const uint8_t* info_table, uint64_t info_len, const uint8_t* out, const svt_paste_line* results, svt_paste_info* info,
                                  Block& b)
{
    if (!info || !first_line || (len && !text) || (n_lines && (!results || !out)) || (info_len && !info_table)) return "null argument";
    *info = svt_paste_info();
    if (flags & ~(SVT_PASTE_SUM_QUALS | SVT_PASTE_AFREQ | SVT_PASTE_SAFE | 3u << SVT_PASTE_LAYOUT_SHIFT))
        return "svt_vcf_paste: flags are SVT_PASTE_SUM_QUALS, _AFREQ, _SAFE and a layout";
    if (len > kMaxLine) return "svt_vcf_paste: a block holds less than 2^31 bytes";
    b.text = text;
    b.len = len;
    b.first_line = first_line;
    b.n_inputs = n_inputs;
    b.n_lines = n_lines;
    b.flags = flags & 0xFFu;
    if (!parse_info_table(info_table, info_len, b.info)) return "svt_vcf_paste: info_table is \"V<id>\\n\" or \"F<id>\\n\" per id";
    return nullptr;
}

inline void unpack_counts(uint64_t lo, uint64_t hi, uint32_t* counts)
{
    for (uint32_t a = 0; a < 4; ++a) {
        counts[a] += (uint32_t)(lo >> (16 * a)) & 0xFFFFu;
        counts[4 + a] += (uint32_t)(hi >> (16 * a)) & 0xFFFFu;
    }
}

// the host twin of svt_paste_measure_kernel: line j's result and places[0, n_inputs)
inline void measure_host(const Block& b, uint64_t j, svt_paste_line& r, Place* places)
{
    r = svt_paste_line();
    r.bad_input = kNoInput;
    r.bad_field = kNoField;
    Master m;
    const uint8_t* master = b.line(0, j);
    measure_master(master, b.line_len(0, j), b.flags, m);
    r.flags = m.slow;
    r.qual = m.qual;
    for (uint32_t s = 0; s < b.n_inputs; ++s) {
        Input in;
        measure_input(b.line(s + 1, j), b.line_len(s + 1, j), master, m, b.flags, in);
        r.qual += in.qual;                          // in file order, from the master's value: the order is the contract
        r.flags |= in.slow;
        unpack_counts(in.lo, in.hi, r.counts);
        r.nonref += in.nonref;
        if (in.unequal != kNoField && r.bad_input == kNoInput) {
            r.bad_input = s;
            r.bad_field = in.unequal;
            r.flags |= SVT_PASTE_UNSAFE;
        }
        places[s] = Place{in.part_b, in.part_len, r.part_len};
        r.part_len += in.part_len ? in.part_len + 1 : 0;
    }
}

// ---- what the slow path and the builder of the first columns share: Python's float(), int() and str(float) of the scripts
struct Bad {
    uint32_t file = 0, kind = 0, field = kNoField; // file 0: the master, f: input f - 1
};

// int(token) where it lies inside [-limit, limit]
inline bool py_small_int(const uint8_t* p, uint32_t b, uint32_t e, int64_t limit, int64_t& v)
{
    std::string text;
    if (!py_int_text(p, b, e, text) || text.size() > 12) return false;
    v = std::strtoll(text.c_str(), nullptr, 10);
    return v >= -limit && v <= limit;
}

// Python 2's str(float): %.12g, with ".0" where that looks like an integer
inline std::string py2_str(double v)
{
    if (std::isnan(v)) return "nan";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.12g", v);
    std::string s(buf);
    if (s.find_first_of(".en") == std::string::npos) s += ".0";      // ('e', "inf", "nan": no ".0")
    return s;
}

// The output line's first columns: CHROM .. FILTER with the QUAL the options ask for, INFO (rebuilt under --afreq), FORMAT.
// `counts`: alleles 0 .. the ALT count.  false: `bad` says why
inline bool build_prefix(const Block& b, uint64_t j, double qual_sum, const std::vector<uint64_t>& counts, uint64_t nonref, std::string& out, Bad& bad)
{
    const uint8_t* p = b.line(0, j);
    Scan s;
    scan_line(p, b.line_len(0, j), s);
    const bool afreq = (b.flags & SVT_PASTE_AFREQ) != 0, sum = (b.flags & SVT_PASTE_SUM_QUALS) != 0;
    bad = Bad();
    if (s.cols < (afreq ? 8u : 6u)) {
        bad.kind = SVT_PASTE_BAD_COLUMNS;
        return false;
    }
    // the end of the eighth column, or of the line where it has fewer
    uint32_t tabs = 0, head_end = 0, col7_b = s.n, col6_b = s.n;
    for (head_end = 0; head_end < s.n; ++head_end) {
        if (p[head_end] != '\t') continue;
        if (++tabs == 8) break;
        if (tabs == 6) col6_b = head_end + 1;
        if (tabs == 7) col7_b = head_end + 1;
    }
    Scan f;
    scan_line(b.line(1, j), b.line_len(1, j), f);
    if (f.cols < 9) {
        bad.file = 1;
        bad.kind = SVT_PASTE_BAD_COLUMNS;
        return false;
    }
    out.clear();
    const std::string qual_text = sum ? py2_str(qual_sum) : std::string((const char*)p + s.qual_b, s.qual_e - s.qual_b);
    if (!afreq) {
        out.append((const char*)p, s.qual_b);
        out += qual_text;
        out.append((const char*)p + s.qual_e, head_end - s.qual_e);
    } else {
        out.append((const char*)p, s.chrom_end + 1);
        std::string pos;
        if (!py_int_text(p, s.pos_b, s.pos_end, pos)) {
            bad.kind = SVT_PASTE_BAD_POS;
            return false;
        }
        out += pos;
        out.append((const char*)p + s.pos_end, s.qual_b - s.pos_end);
        double q = 0.0;                             // the pasted QUAL read again: '.' is 0, anything else a float
        const uint8_t* qt = (const uint8_t*)qual_text.data();
        if (!(qual_text.size() == 1 && qt[0] == '.') && !py_float(qt, 0, (uint32_t)qual_text.size(), q)) {
            bad.kind = SVT_PASTE_BAD_QUAL;
            return false;
        }
        out += fixed2(q);
        out.append((const char*)p + s.qual_e, col7_b - s.qual_e);         // FILTER between its tabs
        (void)col6_b;
        // INFO: key=value pairs split at ';', a value cut at its second '='; a later key replaces an earlier one
        std::vector<std::pair<std::string, std::string>> have;
        for (uint32_t at = col7_b; at <= head_end;) {
            uint32_t e = at;
            while (e < head_end && p[e] != ';') ++e;
            uint32_t eq = at;
            while (eq < e && p[eq] != '=') ++eq;
            std::string value = "True";
            if (eq < e) {
                uint32_t eq2 = eq + 1;
                while (eq2 < e && p[eq2] != '=') ++eq2;
                value.assign((const char*)p + eq + 1, eq2 - eq - 1);
            }
            have.emplace_back(std::string((const char*)p + at, eq - at), value);
            at = e + 1;
        }
        uint64_t total = 0;
        for (uint64_t c : counts) total += c;
        std::string af;
        for (size_t a = 1; a < counts.size(); ++a) {
            if (a > 1) af += ',';
            if (total) {
                char buf[40];
                std::snprintf(buf, sizeof buf, "%.4g", (double)counts[a] / (double)total);
                af += buf;
            } else af += '.';
        }
        bool first = true;
        for (const auto& key : b.info) {
            const std::string* value = nullptr;
            std::string own;
            if (key.first == "AF") value = &af;
            else if (key.first == "NSAMP") {
                own = std::to_string(nonref);
                value = &own;
            } else
                for (size_t k = have.size(); k-- && !value;)
                    if (have[k].first == key.first) value = &have[k].second;
            if (!value) continue;
            if (!first) out += ';';
            first = false;
            out += key.first;
            if (!key.second) {
                out += '=';
                out += *value;
            }
        }
    }
    out += '\t';
    out.append((const char*)b.line(1, j) + f.fmt_b, f.fmt_e - f.fmt_b);
    return true;
}

// The whole of line j in plain C++, as the scripts compute it: r, and the line with its newline, or `bad`
inline bool slow_line(const Block& b, uint64_t j, svt_paste_line& r, std::string& line, Bad& bad)
{
    const uint32_t keep = r.flags & kSlowMask;
    r = svt_paste_line();
    r.flags = keep;
    r.bad_input = kNoInput;
    r.bad_field = kNoField;
    bad = Bad();
    const bool afreq = (b.flags & SVT_PASTE_AFREQ) != 0;
    const uint8_t* mp = b.line(0, j);
    Scan m;
    scan_line(mp, b.line_len(0, j), m);
    if (b.line_len(0, j) > kMaxLine || m.cols < (afreq ? 8u : 6u)) {
        bad.kind = SVT_PASTE_BAD_COLUMNS;
        return false;
    }
    if (!py_float(mp, m.qual_b, m.qual_e, r.qual)) {
        bad.kind = SVT_PASTE_BAD_QUAL;
        return false;
    }
    const uint32_t n_alt = count_alts(mp, m);
    std::vector<uint64_t> counts(afreq ? (size_t)n_alt + 1 : 1, 0);
    uint64_t nonref = 0;
    std::string parts;
    for (uint32_t s = 0; s < b.n_inputs; ++s) {
        const uint8_t* p = b.line(s + 1, j);
        Scan in;
        scan_line(p, b.line_len(s + 1, j), in);
        bad.file = s + 1;
        if (b.flags & SVT_PASTE_SAFE) {
            const uint32_t f = first_unequal(p, in, mp, m);
            if (f != kNoField) {
                bad.kind = SVT_PASTE_BAD_UNSAFE;
                bad.field = f;
                return false;
            }
        }
        if (b.line_len(s + 1, j) > kMaxLine || in.cols < (s == 0 ? 9u : 6u)) {       // FORMAT is the first input's; a QUAL is every input's
            bad.kind = SVT_PASTE_BAD_COLUMNS;
            return false;
        }
        double q = 0.0;
        if (!py_float(p, in.qual_b, in.qual_e, q)) {
            bad.kind = SVT_PASTE_BAD_QUAL;
            return false;
        }
        r.qual += q;
        if (!in.part_len) continue;
        parts += '\t';
        parts.append((const char*)p + in.part_b, in.part_len);
        if (!afreq) continue;
        for (uint32_t at = in.part_b, end = in.part_b + in.part_len; at <= end;) {   // every column's first subfield as a GT
            uint32_t ce = at;
            while (ce < end && p[ce] != '\t') ++ce;
            uint32_t ge = at;
            while (ge < ce && p[ge] != ':') ++ge;
            bool dot = false;
            for (uint32_t i = at; i < ge; ++i) dot |= p[i] == '.';
            if (!dot) {
                uint8_t sep = '|';
                for (uint32_t i = at; i < ge; ++i)
                    if (p[i] == '/') sep = '/';
                std::vector<int64_t> alleles;
                for (uint32_t tb = at; tb <= ge;) {
                    uint32_t te = tb;
                    while (te < ge && p[te] != sep) ++te;
                    int64_t v = 0;
                    std::string text;
                    if (!py_int_text(p, tb, te, text)) {
                        bad.kind = SVT_PASTE_BAD_GT;
                        return false;
                    }
                    if (!py_small_int(p, tb, te, (int64_t)n_alt + 1, v) || v > (int64_t)n_alt) {
                        bad.kind = SVT_PASTE_BAD_ALLELE;
                        return false;
                    }
                    alleles.push_back(v);
                    tb = te + 1;
                }
                int64_t total = 0;                  // (all of a GT is read before any of it counts)
                for (int64_t v : alleles) {
                    counts[(size_t)(v < 0 ? v + (int64_t)n_alt + 1 : v)] += 1;      // a negative index counts from the end
                    total += v;
                }
                nonref += total > 0;
            }
            at = ce + 1;
        }
    }
    bad.file = 0;
    for (size_t a = 0; a < counts.size() && a < 8; ++a) r.counts[a] = (uint32_t)counts[a];
    r.nonref = (uint32_t)nonref;
    r.part_len = (uint32_t)parts.size();
    if (!build_prefix(b, j, r.qual, counts, nonref, line, bad)) return false;
    line += parts;
    line += '\n';
    r.line_len = (uint32_t)line.size();
    return true;
}

// What stands between the two launches, and on the host between measure_host and write_host: the marked lines settled by
// slow_line, every other line's first columns built, the line sizes summed.  Returns the 1-based number of the first line
// that cannot be written (with `bad`), else 0
struct Plan {
    std::string prefixes;                           // the unmarked lines' first columns side by side
    std::vector<uint64_t> prefix_off, out_off;     // [n_lines + 1]
    std::vector<std::pair<uint64_t, std::string>> slow;     // the marked lines, whole
    uint64_t host_lines = 0;
};

inline uint64_t plan_block(const Block& b, svt_paste_line* results, Plan& plan, Bad& bad)
{
    const uint64_t n = b.n_lines;
    plan.prefixes.clear();
    plan.slow.clear();
    plan.prefix_off.assign(n + 1, 0);
    plan.out_off.assign(n + 1, 0);
    plan.host_lines = 0;
    std::string text;
    std::vector<uint64_t> counts;
    for (uint64_t j = 0; j < n; ++j) {
        svt_paste_line& r = results[j];
        if (r.flags & kSlowMask) {
            if (!slow_line(b, j, r, text, bad)) return j + 1;
            ++plan.host_lines;
            plan.slow.emplace_back(j, text);
        } else {
            if (r.flags & SVT_PASTE_UNSAFE) {
                bad = Bad();
                bad.file = r.bad_input + 1;
                bad.kind = SVT_PASTE_BAD_UNSAFE;
                bad.field = r.bad_field;
                return j + 1;
            }
            Scan m;
            scan_line(b.line(0, j), b.line_len(0, j), m);
            counts.assign((b.flags & SVT_PASTE_AFREQ) ? (size_t)count_alts(b.line(0, j), m) + 1 : 1, 0);
            for (size_t a = 0; a < counts.size() && a < 8; ++a) counts[a] = r.counts[a];
            if (!build_prefix(b, j, r.qual, counts, r.nonref, text, bad)) return j + 1;
            plan.prefixes += text;
            r.line_len = (uint32_t)(text.size() + r.part_len + 1);
        }
        plan.prefix_off[j + 1] = plan.prefixes.size();
        plan.out_off[j + 1] = plan.out_off[j] + r.line_len;
    }
    return 0;
}

// the host twin of svt_paste_write_kernel: the unmarked lines into out[0, plan.out_off[n_lines])
inline void write_host(const Block& b, const svt_paste_line* results, const Place* places, const Plan& plan, uint8_t* out)
{
    for (uint64_t j = 0; j < b.n_lines; ++j) {
        if (results[j].flags & kSlowMask) continue;
        uint8_t* at = out + plan.out_off[j];
        const uint64_t pre = plan.prefix_off[j + 1] - plan.prefix_off[j];
        std::memcpy(at, plan.prefixes.data() + plan.prefix_off[j], pre);
        at += pre;
        for (uint32_t s = 0; s < b.n_inputs; ++s) {
            const Place& pl = places[j * b.n_inputs + s];
            if (!pl.len) continue;
            at[pl.dst] = '\t';
            std::memcpy(at + pl.dst + 1, b.line(s + 1, j) + pl.src, pl.len);
        }
        out[plan.out_off[j + 1] - 1] = '\n';
    }
}

inline void write_slow(const Plan& plan, uint8_t* out)
{
    for (const auto& l : plan.slow) std::memcpy(out + plan.out_off[l.first], l.second.data(), l.second.size());
}

inline void report(svt_paste_info& info, uint64_t bad_line, const Bad& bad)
{
    info.bad_line = bad_line;
    info.bad_file = bad.file;
    info.bad_kind = bad.kind;
    info.bad_field = bad.field;
}

// one block on the host: the line table, the twin of both kernels around plan_block
inline const char* paste_host(Block& b, std::vector<svt_tbx_line>& table, svt_paste_line* results, uint8_t* out, uint64_t capacity, svt_paste_info& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    b.lines = table.data();
    b.n_table = table.size();
    if (const char* why = check_block(b)) return why;
    std::vector<Place> places(b.n_lines * b.n_inputs);
    for (uint64_t j = 0; j < b.n_lines; ++j) measure_host(b, j, results[j], places.data() + j * b.n_inputs);
    Plan plan;
    Bad bad;
    if (const uint64_t bad_line = plan_block(b, results, plan, bad)) {
        report(info, bad_line, bad);
        return nullptr;
    }
    info.host_lines = plan.host_lines;
    info.out_len = plan.out_off[b.n_lines];
    if (info.out_len > capacity) return "svt_vcf_paste: capacity is below the pasted text";
    write_host(b, results, places.data(), plan, out);
    write_slow(plan, out);
    return nullptr;
}

}  // namespace paste
}  // namespace svt
#endif  // SVT_VCF_PASTE_H

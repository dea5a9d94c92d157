// svt_vcf_update_info.h -- PE, SR, SU and MSQ of a cohort VCF's lines from the genotyper's per-sample evidence: the per-line rule,
// the host twin of the kernel, the plain C++ of the lines outside the rule's envelope and the writer of the output text
// (include/svtyper_reads.h: svt_update_info_line).
//
// ONE piece of source for both places that run the rule, as svt_vcf_classify.h is: check_head and parse_sample are compiled for
// the host (fast_line, any C++17 compiler: this is where they are proven against goldens made from the reference's
// scripts/update_info.py, and sanitised) and for the device (svt_vcf_update_info_kernel.h, one workgroup per line, lanes over
// samples).  Every load is checked against the line's length.
//
// What the script does with a line: over the header's samples in order it adds int(AP) and int(AS), and float(SQ) of every sample
// whose GT is neither "0/0" nor "./."; INFO's PE, SR, SU (their sum) and MSQ (the mean SQ, '%0.2f', or ".") are set and the line
// is written again field by field (QUAL '%0.2f', INFO and FORMAT in the header's order).
//
// The envelope of the rule: at least ten columns, POS of digits, QUAL "." or inside bcf::double_exact, FORMAT with GT first and
// the header's keys in the header's order, AP and AS among them, one column per sample of the header, every column with exactly
// FORMAT's fields (the sample part of the output is then a slice of the input), AP and AS of one to nine digits, the SQ of a
// positive sample inside bcf::double_exact, 1 to kCapacity samples.  INFO is no part of it: no engine reads INFO for the record,
// and the writer rebuilds it in plain C++ for every line.  Anything else marks the line (SVT_UPDATE_INFO_SLOW_*): nothing is
// guessed, slow_line decides it in plain C++ with strtod and either computes the script's values or names its error.
//
// The order of the double-precision sum is part of the contract: sum_sq starts at +0.0 and takes the positive samples' SQ in
// sample order, on both engines (the kernel adds +0.0 for every other sample, which cannot change such a sum).
#ifndef SVT_VCF_UPDATE_INFO_H
#define SVT_VCF_UPDATE_INFO_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"
#include "svt_vcf_classify.h"

namespace svt {
namespace update_info {

constexpr uint32_t kCapacity = SVT_UPDATE_INFO_CAPACITY, kBlock = 256, kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxCountDigits = 9;             // 4 096 samples of nine digits each stay far below 2^63
// (classify::parse_variant names the errors of a line's first columns and of FORMAT: the two sets of kinds agree there)
static_assert(SVT_UPDATE_INFO_BAD_COLUMNS == SVT_CLASSIFY_BAD_COLUMNS && SVT_UPDATE_INFO_BAD_POS == SVT_CLASSIFY_BAD_POS &&
                  SVT_UPDATE_INFO_BAD_QUAL == SVT_CLASSIFY_BAD_QUAL && SVT_UPDATE_INFO_BAD_FORMAT == SVT_CLASSIFY_BAD_FORMAT,
              "svt_update_info_report and svt_classify_info name a line's first columns alike");

using classify::bytes_are;
using classify::table_index;
using paste::is_digit;
using paste::is_space;

struct Params {
    uint32_t n_samples, format_len;
};

SVT_HD uint32_t stripped_length(const uint8_t* p, uint64_t len)
{
    uint32_t n = len > paste::kMaxLine ? paste::kMaxLine : (uint32_t)len;
    while (n && is_space(p[n - 1])) --n;
    return n;
}

// where the first nine tabs of a right-stripped line stand: tab[0 .. count)
struct Tabs {
    uint32_t tab[9];                                // (indexed by unrolled constants only)
    uint32_t count;
};

SVT_HD void find_tabs(const uint8_t* p, uint32_t n, Tabs& t)
{
    t.count = 0;
    uint32_t at = 0;
#pragma unroll
    for (uint32_t c = 0; c < 9; ++c) {
        t.tab[c] = n;
        if (t.count != c) continue;
        while (at < n && p[at] != '\t') ++at;
        if (at < n) {
            t.tab[c] = at++;
            ++t.count;
        }
    }
}

// what the first nine columns give
struct Head {
    uint32_t n;                                     // the line's length without its trailing blanks
    uint32_t samples_b;                             // behind the ninth tab (n: no tenth column)
    uint32_t n_fmt, ap_i, as_i, sq_i;               // FORMAT's fields; where AP, AS and SQ stand among them (kNone: nowhere)
    uint32_t slow;
};

SVT_HD void check_head(const uint8_t* p, uint32_t n, bool too_long, const Tabs& t, const uint8_t* table, uint32_t table_len, Head& h)
{
    h.n = h.samples_b = n;
    h.n_fmt = h.slow = 0;
    h.ap_i = h.as_i = h.sq_i = kNone;
    if (too_long || t.count < 8) {                  // fewer than nine columns
        h.slow = SVT_UPDATE_INFO_SLOW_HEAD;
        return;
    }
    if (t.count == 9) h.samples_b = t.tab[8] + 1;
    const uint32_t pos_b = t.tab[0] + 1, pos_e = t.tab[1], qual_b = t.tab[4] + 1, qual_e = t.tab[5];
    bool digits = pos_e > pos_b && pos_e - pos_b <= 18;
    for (uint32_t i = pos_b; i < pos_e; ++i) digits = digits && is_digit(p[i]);
    if (!digits) h.slow |= SVT_UPDATE_INFO_SLOW_HEAD;
    double qual;
    if (!bcf::is_dot(p, qual_b, qual_e) && bcf::double_exact(p, qual_b, qual_e, qual)) h.slow |= SVT_UPDATE_INFO_SLOW_HEAD;
    const uint32_t fmt_b = t.tab[7] + 1, fmt_e = t.count == 9 ? t.tab[8] : n;
    uint32_t last = kNone;                          // FORMAT: GT, then the header's keys in the header's order
    for (uint32_t b = fmt_b; b <= fmt_e;) {
        uint32_t e = b;
        while (e < fmt_e && p[e] != ':') ++e;
        const uint32_t k = table_index(table, table_len, p, b, e);
        if (k == kNone || (last == kNone ? k != 0 : k <= last)) h.slow |= SVT_UPDATE_INFO_SLOW_FORMAT;
        last = k;
        if (bytes_are(p, b, e, "AP", 2)) h.ap_i = h.n_fmt;
        if (bytes_are(p, b, e, "AS", 2)) h.as_i = h.n_fmt;
        if (bytes_are(p, b, e, "SQ", 2)) h.sq_i = h.n_fmt;
        ++h.n_fmt;
        b = e + 1;
    }
    if (h.ap_i == kNone || h.as_i == kNone) h.slow |= SVT_UPDATE_INFO_SLOW_KEYS;
}

// one to kMaxCountDigits digits
SVT_HD bool small_count(const uint8_t* p, uint32_t b, uint32_t e, uint32_t& v)
{
    v = 0;
    if (e == b || e - b > kMaxCountDigits) return false;
    for (uint32_t i = b; i < e; ++i) {
        if (!is_digit(p[i])) return false;
        v = v * 10 + (p[i] - '0');
    }
    return true;
}

// what one sample column p[b, e) gives
struct Sample {
    double sq;                                      // +0.0 where the sample is not positive
    uint32_t ap, as, positive, slow;
};

SVT_HD void parse_sample(const uint8_t* p, uint32_t b, uint32_t e, const Head& h, Sample& s)
{
    s.sq = 0.0;
    s.ap = s.as = s.slow = 0;
    s.positive = 1;
    uint32_t idx = 0, sq_b = e, sq_e = e;
    bool has_sq = false;
    for (uint32_t at = b; at <= e; ++idx) {
        uint32_t fe = at;
        while (fe < e && p[fe] != ':') ++fe;
        if (idx == 0) s.positive = !(bytes_are(p, at, fe, "0/0", 3) || bytes_are(p, at, fe, "./.", 3));
        else if (idx == h.ap_i) {
            if (!small_count(p, at, fe, s.ap)) s.slow |= SVT_UPDATE_INFO_SLOW_TOKEN;
        } else if (idx == h.as_i) {
            if (!small_count(p, at, fe, s.as)) s.slow |= SVT_UPDATE_INFO_SLOW_TOKEN;
        } else if (idx == h.sq_i) {
            sq_b = at;
            sq_e = fe;
            has_sq = true;
        }
        at = fe + 1;
    }
    if (idx != h.n_fmt) s.slow |= SVT_UPDATE_INFO_SLOW_SAMPLE;
    if (s.positive) {
        if (h.sq_i == kNone) s.slow |= SVT_UPDATE_INFO_SLOW_KEYS;
        else if (!has_sq || bcf::double_exact(p, sq_b, sq_e, s.sq)) {
            s.slow |= SVT_UPDATE_INFO_SLOW_TOKEN;
            s.sq = 0.0;
        }
    }
}

SVT_HD uint64_t bits_of(double v)
{
    union { double d; uint64_t u; } x;
    x.d = v;
    return x.u;
}

SVT_HD double double_of(uint64_t u)
{
    union { double d; uint64_t u; } x;
    x.u = u;
    return x.d;
}

SVT_HD svt_update_info_line marked_record(uint32_t flags)
{
    svt_update_info_line r;
    r.pe = r.sr = 0;
    r.sum_sq = 0;
    r.num_pos = r.reserved = 0;
    r.route = flags ? SVT_UPDATE_INFO_PLAIN : SVT_UPDATE_INFO_RULE;
    r.flags = flags;
    return r;
}

}  // namespace update_info
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace svt {
namespace update_info {

using classify::Bad;
using classify::Block;                              // the text under its line table, the header's FORMAT ids, (the writer) its INFO ids
using classify::Variant;

inline const char* take_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                                  const svt_update_info_line* results, const uint64_t* n_lines, svt_update_info_report* info, Block& b)
{
    if (!info || !n_lines || !results || (len && !text) || !format_table) return "null argument";
    *info = svt_update_info_report();
    if (len > paste::kMaxLine) return "svt_vcf_update_info: a block holds less than 2^31 bytes";
    if (format_len > 0xFFFFu || !classify::parse_format_table(format_table, format_len, b.formats))
        return "svt_vcf_update_info: format_table is \"<id>\\n\" per id, GT first";
    b.text = text;
    b.len = len;
    b.format_table = format_table;
    b.pr.n_samples = n_samples;
    b.pr.format_len = (uint32_t)format_len;
    return nullptr;
}

// The host twin of svt_update_info_kernel for one line: its record, the marks the kernel would set included.  A marked line's
// values are slow_line's
inline svt_update_info_line fast_line(const Block& b, const uint8_t* p, uint64_t len)
{
    const uint32_t n_line = stripped_length(p, len), n = b.pr.n_samples;
    Tabs t;
    find_tabs(p, n_line, t);
    Head h;
    check_head(p, n_line, len > paste::kMaxLine, t, b.format_table, b.pr.format_len, h);
    if (h.slow) return marked_record(h.slow);
    if (!n || n > kCapacity) return marked_record(SVT_UPDATE_INFO_SLOW_CAPACITY);
    std::vector<uint32_t> starts;
    if (h.samples_b < h.n) {
        starts.push_back(h.samples_b);
        for (uint32_t i = h.samples_b; i < h.n; ++i)
            if (p[i] == '\t') starts.push_back(i + 1);
    }
    if (starts.size() != n) return marked_record(SVT_UPDATE_INFO_SLOW_COLUMNS);
    svt_update_info_line r = marked_record(0);
    double sum_sq = 0.0;
    uint32_t slow = 0;
    for (uint32_t s = 0; s < n; ++s) {
        Sample sm;
        parse_sample(p, starts[s], s + 1 < n ? starts[s + 1] - 1 : h.n, h, sm);
        slow |= sm.slow;
        r.pe += sm.ap;
        r.sr += sm.as;
        r.num_pos += sm.positive;
        if (sm.positive) sum_sq += sm.sq;           // in sample order: the order is the contract
    }
    if (slow) return marked_record(slow);
    r.sum_sq = bits_of(sum_sq);
    return r;
}

// int(token) of Python 2 inside int64
inline bool py_int64(const std::string& token, int64_t& v, Bad& bad)
{
    std::string text;
    bad.text = token;
    if (!paste::py_int_text((const uint8_t*)token.data(), 0, (uint32_t)token.size(), text)) {
        bad.kind = SVT_UPDATE_INFO_BAD_NUMBER;
        return false;
    }
    errno = 0;
    v = std::strtoll(text.c_str(), nullptr, 10);
    if (errno == ERANGE) {
        bad.kind = SVT_UPDATE_INFO_BAD_OVERFLOW;
        return false;
    }
    return true;
}

// genotype(sample).get_format(key)
inline const std::string* sample_field(const Block& b, const Variant& v, uint32_t s, const char* key, Bad& bad)
{
    const uint32_t k = classify::format_index(b, key);
    bad.sample = s;
    if (k == kNone || !v.has[s][k]) {
        bad.kind = SVT_UPDATE_INFO_BAD_KEY;
        bad.text = key;
        return nullptr;
    }
    return &v.value[s][k];
}

// Variant(v, vcf) of the script in its order, the errors of a line with fewer than eight columns included: the script reads
// POS and QUAL before it counts the columns
inline bool parse_line(const Block& b, const uint8_t* p, uint64_t len, bool samples, Variant& v, Bad& bad)
{
    const uint32_t n = stripped_length(p, len);
    std::vector<std::pair<uint32_t, uint32_t>> col;
    classify::split(p, 0, n, '\t', col);
    if (len <= paste::kMaxLine && col.size() < 8) {
        std::string text;
        double q = 0.0;
        bad.kind = SVT_UPDATE_INFO_BAD_COLUMNS;
        if (col.size() < 2) return false;
        if (!paste::py_int_text(p, col[1].first, col[1].second, text)) {
            bad.kind = SVT_UPDATE_INFO_BAD_POS;
            bad.text = classify::bytes(p, col[1].first, col[1].second);
            return false;
        }
        if (col.size() < 6) return false;
        if (!bcf::is_dot(p, col[5].first, col[5].second) && !paste::py_float(p, col[5].first, col[5].second, q)) {
            bad.kind = SVT_UPDATE_INFO_BAD_QUAL;
            bad.text = classify::bytes(p, col[5].first, col[5].second);
            return false;
        }
        if (col.size() == 7) bad.kind = SVT_UPDATE_INFO_BAD_EIGHT;
        return false;
    }
    return classify::parse_variant(b, p, len, samples, v, bad);     // (the kinds of both carry the same numbers)
}

// the sums of a parsed line, looked up in the script's order
inline bool sums(const Block& b, const Variant& v, svt_update_info_line& r, Bad& bad)
{
    double sum_sq = 0.0;
    for (uint32_t s = 0; s < b.pr.n_samples; ++s) {
        for (int which = 0; which < 2; ++which) {
            const std::string* token = sample_field(b, v, s, which ? "AS" : "AP", bad);
            int64_t value = 0;
            if (!token || !py_int64(*token, value, bad)) return false;
            if (__builtin_add_overflow(which ? r.sr : r.pe, value, which ? &r.sr : &r.pe)) {
                bad.kind = SVT_UPDATE_INFO_BAD_OVERFLOW;
                return false;
            }
        }
        const std::string& gt = v.value[s][0];
        if (gt == "0/0" || gt == "./.") continue;
        const std::string* token = sample_field(b, v, s, "SQ", bad);
        if (!token) return false;
        double sq = 0.0;
        bad.text = *token;
        if (!paste::py_float((const uint8_t*)token->data(), 0, (uint32_t)token->size(), sq)) {
            bad.kind = SVT_UPDATE_INFO_BAD_NUMBER;
            return false;
        }
        if (!std::isfinite(sq)) {
            bad.kind = SVT_UPDATE_INFO_BAD_NONFINITE;
            return false;
        }
        ++r.num_pos;
        sum_sq += sq;
    }
    int64_t su;
    if (__builtin_add_overflow(r.pe, r.sr, &su)) {
        bad.kind = SVT_UPDATE_INFO_BAD_OVERFLOW;
        bad.sample = kNone;
        bad.text = "SU";
        return false;
    }
    r.sum_sq = bits_of(sum_sq);
    bad = Bad();
    return true;
}

// The whole of one line in plain C++, as the script computes it, in the script's order: r (the marks kept), or `bad`
inline bool slow_line(const Block& b, const uint8_t* p, uint64_t len, svt_update_info_line& r, Bad& bad)
{
    r = marked_record(r.flags & SVT_UPDATE_INFO_SLOW);
    r.route = SVT_UPDATE_INFO_PLAIN;
    bad = Bad();
    Variant v;
    return parse_line(b, p, len, true, v, bad) && sums(b, v, r, bad);
}

// what one line's record makes of it, appended to `out`: get_var_string with PE, SR, SU and MSQ set.  An unmarked line's FORMAT
// and sample columns are the input's
inline bool write_line(const Block& b, const uint8_t* p, uint64_t len, const svt_update_info_line& r, std::string& out, Bad& bad)
{
    bad = Bad();
    const bool marked = (r.flags & SVT_UPDATE_INFO_SLOW) != 0;
    Variant v;
    if (!parse_line(b, p, len, marked, v, bad)) return false;
    std::string tail;
    if (marked) tail = classify::generic_tail(b, v);
    else if (v.col.size() > 9) tail = classify::bytes(p, v.col[8].first, stripped_length(p, len));
    else {
        bad.kind = SVT_UPDATE_INFO_BAD_COLUMNS;     // (a record that is not this line's)
        return false;
    }
    int64_t su = 0;
    if (__builtin_add_overflow(r.pe, r.sr, &su)) {
        bad.kind = SVT_UPDATE_INFO_BAD_OVERFLOW;
        return false;
    }
    v.set_info("PE", std::to_string(r.pe));
    v.set_info("SR", std::to_string(r.sr));
    v.set_info("SU", std::to_string(su));
    v.set_info("MSQ", r.num_pos ? paste::fixed2(double_of(r.sum_sq) / (double)r.num_pos) : std::string("."));
    classify::var_string(b, v, tail, out);
    return true;
}

inline void report(svt_update_info_report& info, uint64_t bad_line, const Bad& bad)
{
    info.bad_line = bad_line;
    info.bad_kind = bad.kind;
    info.bad_sample = bad.sample;
    std::memset(info.bad_text, 0, sizeof info.bad_text);
    std::memcpy(info.bad_text, bad.text.data(), std::min(bad.text.size(), sizeof info.bad_text - 1));
}

// What follows the rule on both engines: the marked lines settled by slow_line, counted.  Returns the 1-based number of the
// first line the script dies on (with `bad`), else 0
inline uint64_t settle_block(const Block& b, svt_update_info_line* results, svt_update_info_report& info, Bad& bad)
{
    for (uint64_t j = 0; j < b.n_table; ++j) {
        if (!(results[j].flags & SVT_UPDATE_INFO_SLOW)) continue;
        if (!slow_line(b, b.text + b.lines[j].off, b.lines[j].len, results[j], bad)) return j + 1;
        ++info.host_lines;
    }
    return 0;
}

inline const char* update_info_host(Block& b, std::vector<svt_tbx_line>& table, svt_update_info_line* results, uint64_t capacity, uint64_t* n_lines,
                                    svt_update_info_report& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    b.lines = table.data();
    b.n_table = table.size();
    *n_lines = table.size();
    if (table.size() > capacity) return "svt_vcf_update_info: capacity is below the number of lines";
    for (uint64_t j = 0; j < b.n_table; ++j) results[j] = update_info::fast_line(b, b.text + table[j].off, table[j].len);
    Bad bad;
    if (const uint64_t bad_line = settle_block(b, results, info, bad)) report(info, bad_line, bad);
    return nullptr;
}

// the writer's entry: the block's output into `out`, out_off[0 .. n_lines]
inline const char* write_block(Block& b, std::vector<svt_tbx_line>& table, const svt_update_info_line* results, uint64_t n_lines, uint64_t* out_off,
                               std::string& out, svt_update_info_report& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    if (table.size() != n_lines) return "svt_vcf_update_info_write: one record per line of the text";
    out.clear();
    out_off[0] = 0;
    Bad bad;
    for (uint64_t j = 0; j < n_lines; ++j) {
        if (!write_line(b, b.text + table[j].off, table[j].len, results[j], out, bad)) {
            report(info, j + 1, bad);
            out.resize(out_off[j]);
            for (uint64_t k = j; k < n_lines; ++k) out_off[k + 1] = out_off[j];
            break;
        }
        out_off[j + 1] = out.size();
    }
    info.out_len = out.size();
    return nullptr;
}

}  // namespace update_info
}  // namespace svt
#endif  // SVT_VCF_UPDATE_INFO_H

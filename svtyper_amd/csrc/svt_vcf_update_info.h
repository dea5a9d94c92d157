// svt_vcf_update_info.h -- PE, SR, SU and MSQ of a cohort VCF's lines from the genotyper's per-sample evidence: the per-line rule,
// the host twin of the kernel, the plain C++ of the lines outside the rule's envelope and the writer of the output text
// (include/svtyper_reads.h: svt_update_info_line).
//
// ONE piece of source for both places that run the rule, as svt_vcf_classify.h is: check_head and parse_sample are compiled for
// the host (fast_line, any C++17 compiler: this is where they are proven against goldens made from the reference's
// scripts/update_info.py, and sanitised) and for the device (svt_vcf_update_info_kernel.h, one workgroup per line, lanes over
// samples).  Every load is checked against the line's length.  What a cohort line is to every rule (its tabs, POS, QUAL and
// FORMAT, the script's Variant, the drivers) is svt_vcf_cohort_line.h's.
//
// What the script does with a line: over the header's samples in order it adds int(AP) and int(AS), and float(SQ) of every sample
// whose GT is neither "0/0" nor "./."; INFO's PE, SR, SU (their sum) and MSQ (the mean SQ, '%0.2f', or ".") are set and the line
// is written again field by field (QUAL '%0.2f', INFO and FORMAT in the header's order).
//
// The envelope of the rule: at least ten columns, the head as cohort::check_head wants it with AP and AS in FORMAT, one column per
// sample of the header, every column with exactly FORMAT's fields (the sample part of the output is then a slice of the input), AP
// and AS of one to nine digits, the SQ of a positive sample inside bcf::double_exact, 1 to kCapacity samples.  INFO is no part of
// it: no engine reads INFO for the record, and the writer rebuilds it in plain C++ for every line.  Anything else marks the line
// (SVT_UPDATE_INFO_SLOW_*): nothing is guessed, slow_line decides it in plain C++ with strtod and either computes the script's
// values or names its error.
//
// The order of the double-precision sum is part of the contract: sum_sq starts at +0.0 and takes the positive samples' SQ in
// sample order, on both engines (the kernel adds +0.0 for every other sample, which cannot change such a sum).
#ifndef SVT_VCF_UPDATE_INFO_H
#define SVT_VCF_UPDATE_INFO_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"
#include "svt_vcf_cohort_line.h"

namespace svt {
namespace update_info {

constexpr uint32_t kCapacity = SVT_UPDATE_INFO_CAPACITY;
constexpr uint32_t kMaxCountDigits = 9;             // 4 096 samples of nine digits each stay far below 2^63
constexpr uint32_t kAp = 0, kAs = 1, kSq = 2;       // Head::key_at: where AP, AS and SQ stand in FORMAT

using cohort::bytes_are;
using cohort::is_digit;
using cohort::kBlock;
using cohort::kNone;
using cohort::Tabs;

struct Params {
    uint32_t n_samples, format_len;
};

struct Head : cohort::Head {};                     // (its own type: the drivers find the rule's check_head by it)

SVT_HD void check_head(const uint8_t* p, uint32_t n, bool too_long, const Tabs& t, const uint8_t* table, uint32_t table_len, Head& h)
{
    cohort::begin_head(n, t, h);
    if (too_long || t.count < 8) {                  // fewer than nine columns
        h.slow = SVT_UPDATE_INFO_SLOW_HEAD;
        return;
    }
    cohort::check_head(p, t, table, table_len, SVT_UPDATE_INFO_SLOW_HEAD, SVT_UPDATE_INFO_SLOW_FORMAT, "APASSQ", 3, h);
    if (h.key_at[kAp] == kNone || h.key_at[kAs] == kNone) h.slow |= SVT_UPDATE_INFO_SLOW_KEYS;
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
    uint32_t sq_b = e, sq_e = e;
    bool has_sq = false;
    const uint32_t fields = cohort::walk_fields(p, b, e, ':', [&](uint32_t idx, uint32_t at, uint32_t fe) {
        if (idx == 0) s.positive = !(bytes_are(p, at, fe, "0/0", 3) || bytes_are(p, at, fe, "./.", 3));
        else if (idx == h.key_at[kAp]) {
            if (!small_count(p, at, fe, s.ap)) s.slow |= SVT_UPDATE_INFO_SLOW_TOKEN;
        } else if (idx == h.key_at[kAs]) {
            if (!small_count(p, at, fe, s.as)) s.slow |= SVT_UPDATE_INFO_SLOW_TOKEN;
        } else if (idx == h.key_at[kSq]) {
            sq_b = at;
            sq_e = fe;
            has_sq = true;
        }
    });
    if (fields != h.n_fmt) s.slow |= SVT_UPDATE_INFO_SLOW_SAMPLE;
    if (s.positive) {
        if (h.key_at[kSq] == kNone) s.slow |= SVT_UPDATE_INFO_SLOW_KEYS;
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

using cohort::Bad;
using cohort::Variant;
using cohort::write_block;

struct Block : cohort::Block {
    static constexpr const char* kName = "svt_vcf_update_info";
    static constexpr const char* kCapacityWhy = "svt_vcf_update_info: capacity is below the number of lines";
    static constexpr const char* kWriteWhy = "svt_vcf_update_info_write: one record per line of the text";
    static constexpr const char* kLengthWhy = "svt_vcf_update_info: a block holds less than 2^31 bytes";
    static constexpr const char* kFormatWhy = "svt_vcf_update_info: format_table is \"<id>\\n\" per id, GT first";
    Params pr = Params();
};

inline const char* take_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                                  const svt_update_info_line* results, const uint64_t* n_lines, svt_update_info_report* info, Block& b)
{
    return cohort::take_block_arguments(text, len, n_samples, format_table, format_len, n_lines && results, info, b);
}

// The host twin of svt_update_info_kernel for one line: its record, the marks the kernel would set included.  A marked line's
// values are slow_line's
inline svt_update_info_line fast_line(const Block& b, const uint8_t* p, uint64_t len)
{
    const uint32_t n = b.pr.n_samples;
    const Head h = cohort::head_of<Head>(b, p, len);
    if (h.slow) return marked_record(h.slow);
    if (!n || n > kCapacity) return marked_record(SVT_UPDATE_INFO_SLOW_CAPACITY);
    std::vector<uint32_t> starts;
    cohort::column_starts(p, h, starts);
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
    if (!cohort::py_int_text((const uint8_t*)token.data(), 0, (uint32_t)token.size(), text)) {
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
    const uint32_t k = cohort::format_index(b, key);
    bad.sample = s;
    if (k == kNone || !v.has[s][k]) {
        bad.kind = SVT_UPDATE_INFO_BAD_KEY;
        bad.text = key;
        return nullptr;
    }
    return &v.value[s][k];
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
        if (!cohort::py_float((const uint8_t*)token->data(), 0, (uint32_t)token->size(), sq)) {
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
    return cohort::parse_variant(b, b.pr.n_samples, p, len, true, true, v, bad) && sums(b, v, r, bad);
}

// what one line's record makes of it, appended to `out`: get_var_string with PE, SR, SU and MSQ set.  An unmarked line's FORMAT
// and sample columns are the input's
inline bool write_line(const Block& b, const uint8_t* p, uint64_t len, const svt_update_info_line& r, std::string& out, Bad& bad)
{
    bad = Bad();
    const bool marked = (r.flags & SVT_UPDATE_INFO_SLOW) != 0;
    Variant v;
    if (!cohort::parse_variant(b, b.pr.n_samples, p, len, marked, true, v, bad)) return false;
    std::string tail;
    if (marked) tail = cohort::generic_tail(b, v);
    else if (v.col.size() > 9) tail = cohort::bytes(p, v.col[8].first, cohort::stripped_length(p, len));
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
    v.set_info("MSQ", r.num_pos ? cohort::fixed2(double_of(r.sum_sq) / (double)r.num_pos) : std::string("."));
    cohort::var_string(b, v, tail, out);
    return true;
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
    return cohort::rule_host(b, table, results, capacity, n_lines, info);
}

}  // namespace update_info
}  // namespace svt
#endif  // SVT_VCF_UPDATE_INFO_H

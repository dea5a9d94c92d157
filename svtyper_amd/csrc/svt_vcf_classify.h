// svt_vcf_classify.h -- the read-depth classifier of DEL and DUP lines: the per-line rule, the host twin of the kernel, the plain
// C++ of the lines outside the rule's envelope and the writer of the output text (include/svtyper_reads.h:
// svt_classify_line).
//
// ONE piece of source for both places that run the rule, as svt_vcf_paste.h is: scan_head, parse_sample, the order-preserving
// keys, supports, finish_low and finish_high are compiled for the host (fast_line, any C++17 compiler: this is where they are
// proven against goldens made from the reference's scripts/sv_classifier.py, and sanitised) and for the device
// (svt_vcf_classify_kernel.h, one workgroup per line, lanes over samples).  Every load is checked against the line's length.
//
// What the script does with a DEL or DUP line: it counts the samples not excluded whose GT is neither "./." nor "0/0"; below
// ten it compares the CN of the carriers with the median and the median absolute deviation of the "0/0" samples' CN; from ten
// on it regresses CN on AB.  A supported line is written again field by field, an unsupported one as two BND lines.
//
// The envelope of the rule: at least ten columns, POS of digits, QUAL "." or inside bcf::double_exact, one SVTYPE item, FORMAT
// with GT first and the header's keys in the header's order, one column per sample of the header, every column with exactly
// FORMAT's fields, every CN and every AB that is not "." inside bcf::double_exact, 1 to kCapacity samples, on X and Y every
// sample with a gender, and the keys the route reads in FORMAT.  Anything else marks the line (SVT_CLASSIFY_SLOW_*): nothing is
// guessed, slow_line decides it in plain C++ with strtod and either computes the script's values or names its error.
//
// The order of the double-precision sums is part of the contract (slope and r2 are bit-identical between the engines): sample s
// adds into partial s % 256 in sample order, the 256 partials are joined per 64 by halving (p[l] += p[l + d], d = 32 .. 1) and
// the four results as (w0 + w1) + (w2 + w3): what 256 lanes, an xor butterfly per wavefront and one exchange through LDS give.
#ifndef SVT_VCF_CLASSIFY_H
#define SVT_VCF_CLASSIFY_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"
#include "svt_vcf_paste.h"

namespace svt {
namespace classify {

constexpr uint32_t kCapacity = SVT_CLASSIFY_CAPACITY, kBlock = 256, kNone = 0xFFFFFFFFu;
constexpr uint32_t kMinPosForRegression = 10;
constexpr uint32_t kGtMissing = 0, kGtRef = 1, kGtHet = 2, kGtHom = 3, kGtOther = 4;
constexpr double kNearBand = 1e-9;

using paste::is_digit;
using paste::is_space;

struct Params {
    double slope_threshold, rsquared_threshold;
    uint32_t n_samples, format_len;
};

SVT_HD bool bytes_are(const uint8_t* p, uint32_t b, uint32_t e, const char* w, uint32_t n)
{
    if (e - b != n) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (p[b + i] != (uint8_t)w[i]) return false;
    return true;
}

// the index of p[b, e) among the "<id>\n" of the table, kNone where it is none of them
SVT_HD uint32_t table_index(const uint8_t* table, uint32_t table_len, const uint8_t* p, uint32_t b, uint32_t e)
{
    uint32_t k = 0;
    for (uint32_t at = 0; at < table_len; ++k) {
        uint32_t end = at;
        while (end < table_len && table[end] != '\n') ++end;
        if (end - at == e - b) {
            uint32_t i = 0;
            while (i < e - b && table[at + i] == p[b + i]) ++i;
            if (i == e - b) return k;
        }
        at = end + 1;
    }
    return kNone;
}

// what the first nine columns of one right-stripped line give
struct Head {
    uint32_t n;                                     // the line's length without its trailing blanks
    uint32_t samples_b;                             // behind the ninth tab (n: no tenth column)
    uint32_t svtype;                                // of the first item "SVTYPE=": 0 neither, 1 DEL, 2 DUP
    uint32_t sex;                                   // CHROM is exactly X or Y
    uint32_t n_fmt, cn_i, ab_i;                     // FORMAT's fields; where CN and AB stand among them (kNone: nowhere)
    uint32_t slow;
};

SVT_HD void scan_head(const uint8_t* p, uint64_t len, const uint8_t* table, uint32_t table_len, Head& h)
{
    uint32_t n = len > paste::kMaxLine ? paste::kMaxLine : (uint32_t)len;
    while (n && is_space(p[n - 1])) --n;
    h.n = h.samples_b = n;
    h.svtype = h.sex = h.n_fmt = h.slow = 0;
    h.cn_i = h.ab_i = kNone;
    uint32_t cb[9], ce[9], cols = 0, at = 0;       // (indexed by unrolled constants only)
    bool more = true;
#pragma unroll
    for (uint32_t c = 0; c < 9; ++c) {
        cb[c] = ce[c] = n;
        if (!more) continue;
        uint32_t e = at;
        while (e < n && p[e] != '\t') ++e;
        cb[c] = at;
        ce[c] = e;
        ++cols;
        if (e == n) more = false;
        else at = e + 1;
    }
    if (more) h.samples_b = at;
    if (len > paste::kMaxLine || cols < 8) {        // (the script's IndexError: slow_line names it)
        h.slow = SVT_CLASSIFY_SLOW_HEAD;
        h.svtype = 1;
        return;
    }
    // INFO: the first item that starts "SVTYPE=" decides; a second item of that key can change the type behind it
    uint32_t keyed = 0;
    bool found = false;
    for (uint32_t b = cb[7]; b <= ce[7];) {
        uint32_t e = b, eq = kNone;
        for (; e < ce[7] && p[e] != ';'; ++e)
            if (p[e] == '=' && eq == kNone) eq = e;
        const uint32_t key_e = eq == kNone ? e : eq;
        if (bytes_are(p, b, key_e, "SVTYPE", 6)) {
            ++keyed;
            if (eq != kNone && !found) {
                found = true;
                uint32_t ve = eq + 1;
                while (ve < e && p[ve] != '=') ++ve;
                h.svtype = bytes_are(p, eq + 1, ve, "DEL", 3) ? 1u : bytes_are(p, eq + 1, ve, "DUP", 3) ? 2u : 0u;
            }
        }
        b = e + 1;
    }
    if (!h.svtype) return;
    if (keyed > 1) h.slow |= SVT_CLASSIFY_SLOW_HEAD;
    if (!more) h.slow |= SVT_CLASSIFY_SLOW_HEAD;
    h.sex = ce[0] == 1 && (p[0] == 'X' || p[0] == 'Y');
    bool digits = ce[1] > cb[1] && ce[1] - cb[1] <= 18;
    for (uint32_t i = cb[1]; i < ce[1]; ++i) digits = digits && is_digit(p[i]);
    if (!digits) h.slow |= SVT_CLASSIFY_SLOW_HEAD;
    double qual;
    if (!bcf::is_dot(p, cb[5], ce[5]) && bcf::double_exact(p, cb[5], ce[5], qual)) h.slow |= SVT_CLASSIFY_SLOW_HEAD;
    uint32_t last = kNone;                          // FORMAT: GT, then the header's keys in the header's order
    for (uint32_t b = cb[8]; b <= ce[8];) {
        uint32_t e = b;
        while (e < ce[8] && p[e] != ':') ++e;
        const uint32_t k = table_index(table, table_len, p, b, e);
        if (k == kNone || (last == kNone ? k != 0 : k <= last)) h.slow |= SVT_CLASSIFY_SLOW_FORMAT;
        last = k;
        if (bytes_are(p, b, e, "CN", 2)) h.cn_i = h.n_fmt;
        if (bytes_are(p, b, e, "AB", 2)) h.ab_i = h.n_fmt;
        ++h.n_fmt;
        b = e + 1;
    }
}

// what one sample column p[b, e) gives
struct Sample {
    double cn, ab;
    uint32_t gt, slow;
    bool has_ab;                                    // AB is neither "." nor -1
};

SVT_HD void parse_sample(const uint8_t* p, uint32_t b, uint32_t e, const Head& h, Sample& s)
{
    s.cn = s.ab = 0.0;
    s.gt = kGtOther;
    s.slow = 0;
    s.has_ab = false;
    uint32_t idx = 0;
    for (uint32_t at = b; at <= e; ++idx) {
        uint32_t fe = at;
        while (fe < e && p[fe] != ':') ++fe;
        if (idx == 0) {
            if (bytes_are(p, at, fe, "./.", 3)) s.gt = kGtMissing;
            else if (bytes_are(p, at, fe, "0/0", 3)) s.gt = kGtRef;
            else if (bytes_are(p, at, fe, "0/1", 3)) s.gt = kGtHet;
            else if (bytes_are(p, at, fe, "1/1", 3)) s.gt = kGtHom;
        } else if (idx == h.cn_i) {
            if (bcf::double_exact(p, at, fe, s.cn)) s.slow |= SVT_CLASSIFY_SLOW_TOKEN;
        } else if (idx == h.ab_i) {
            if (!bcf::is_dot(p, at, fe)) {
                if (bcf::double_exact(p, at, fe, s.ab)) s.slow |= SVT_CLASSIFY_SLOW_TOKEN;
                s.has_ab = s.ab != -1.0;
            }
        }
        at = fe + 1;
    }
    if (idx != h.n_fmt) s.slow |= SVT_CLASSIFY_SLOW_SAMPLE;
}

// which list of the low-frequency test a sample's CN enters: 1 the list the median is taken of, 2 the carriers, 0 neither.
// `sex_pick`: 0 on an autosome, 1 / 2 where the males / females of X or Y were chosen: the script then overwrites its "0/0"
// list with the chosen sex's "0/1" list and leaves the "0/1" list empty, which is followed here
SVT_HD uint32_t low_list(uint32_t gt, uint32_t sex_pick, bool male, bool female)
{
    if (!sex_pick) return gt == kGtRef ? 1u : (gt == kGtHet || gt == kGtHom) ? 2u : 0u;
    if (!(sex_pick == 1 ? male : female)) return 0;
    return gt == kGtHet ? 1u : gt == kGtHom ? 2u : 0u;
}

// order-preserving 64-bit keys of doubles (no NaN reaches them); -0.0 sorts below 0.0
SVT_HD uint64_t key_of(double v)
{
    union { double d; uint64_t u; } x;
    x.d = v;
    return (x.u >> 63) ? ~x.u : x.u | 0x8000000000000000ull;
}

SVT_HD double value_of(uint64_t k)
{
    union { double d; uint64_t u; } x;
    x.u = (k >> 63) ? k & 0x7FFFFFFFFFFFFFFFull : ~k;
    return x.d;
}

// np.median of n sorted keys, n > 0: the middle one, or (a + b) / 2 of the two middle ones
SVT_HD double median_sorted(const uint64_t* keys, uint32_t n)
{
    if (n & 1) return value_of(keys[n / 2]);
    return (value_of(keys[n / 2 - 1]) + value_of(keys[n / 2])) / 2.0;
}

SVT_HD bool supports(double cn, double median, double mad, bool del)
{
    double resid = cn - median;
    if (del) resid = -resid;
    return resid > mad * 2.0 && resid > 0.5;
}

SVT_HD void finish_low(svt_classify_line& r)
{
    r.verdict = r.n_ref > 0 && r.n_alt > 0 && (double)r.quorum / (double)r.n_alt > 0.5;
}

SVT_HD bool near_to(double v, double threshold)
{
    const double d = v > threshold ? v - threshold : threshold - v, t = threshold < 0 ? -threshold : threshold;
    return threshold == 0.0 ? d <= kNearBand : d <= kNearBand * t;
}

// the regression's end: the centred sums of the n_regressed samples -> slope, r2, the band and the verdict.  `distinct`: AB and
// CN both have more than one value
SVT_HD void finish_high(svt_classify_line& r, bool has_cn, bool distinct, double sxx, double syy, double sxy, bool del, const Params& pr)
{
    r.verdict = 0;
    r.slope = r.r2 = 0.0;
    if (!has_cn || !distinct) return;
    r.slope = sxy / sxx;
    const double den = sxx * syy;
    r.r2 = den == 0.0 ? 0.0 : (sxy * sxy) / den;
    if (r.r2 > 1.0) r.r2 = 1.0;
    const double signed_slope = del ? -r.slope : r.slope;
    if (near_to(r.r2, pr.rsquared_threshold) || near_to(signed_slope, pr.slope_threshold)) r.flags |= SVT_CLASSIFY_NEAR;
    r.verdict = !(r.r2 < pr.rsquared_threshold) && !(signed_slope < pr.slope_threshold);
}

// the keys the route reads and FORMAT lacks
SVT_HD uint32_t route_keys(uint32_t route, const Head& h)
{
    if (route == SVT_CLASSIFY_LOW) return h.cn_i == kNone ? SVT_CLASSIFY_SLOW_KEYS : 0u;
    return h.cn_i != kNone && h.ab_i == kNone ? SVT_CLASSIFY_SLOW_KEYS : 0u;
}

SVT_HD svt_classify_line empty_record(uint32_t route, uint32_t flags)
{
    svt_classify_line r;
    r.median = r.mad = r.slope = r.r2 = 0.0;
    r.route = route;
    r.verdict = r.n_pos = r.n_ref = r.n_alt = r.quorum = r.n_regressed = 0;
    r.flags = flags;
    return r;
}

}  // namespace classify
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace svt {
namespace classify {

// the 256 partial sums and their fixed join (the header of this file)
struct Tree {
    double p[kBlock];
    Tree() { for (double& v : p) v = 0.0; }
    void add(uint32_t s, double v) { p[s % kBlock] += v; }
    double total()
    {
        for (uint32_t w = 0; w < kBlock; w += 64)
            for (uint32_t d = 32; d; d >>= 1)
                for (uint32_t l = 0; l < d; ++l) p[w + l] += p[w + l + d];
        return (p[0] + p[64]) + (p[128] + p[192]);
    }
};

struct Bad {
    uint32_t kind = 0, sample = kNone;
    std::string text;
};

// one block: the text under its line table, the per-sample tables, the header's FORMAT ids
struct Block {
    const uint8_t* text = nullptr;
    uint64_t len = 0;
    const svt_tbx_line* lines = nullptr;
    uint64_t n_table = 0;
    const uint8_t *male = nullptr, *female = nullptr, *excluded = nullptr, *skip = nullptr;
    const uint8_t* format_table = nullptr;
    Params pr = Params();
    std::vector<std::string> formats;
    std::vector<std::pair<std::string, bool>> info; // (the writer) the header's INFO ids in its order, and whether the Type is Flag
    bool is_male(uint32_t s) const { return male[s] == 1; }
    bool is_female(uint32_t s) const { return female[s] == 1; }
    bool no_gender(uint32_t s) const { return male[s] == SVT_CLASSIFY_NO_GENDER; }
};

inline bool parse_format_table(const uint8_t* p, uint64_t n, std::vector<std::string>& formats)
{
    formats.clear();
    for (uint64_t at = 0; at < n;) {
        const void* nl = std::memchr(p + at, '\n', n - at);
        if (!nl) return false;
        const uint64_t e = (uint64_t)((const uint8_t*)nl - p);
        formats.emplace_back((const char*)p + at, e - at);
        at = e + 1;
    }
    return !formats.empty() && formats[0] == "GT";
}

// ---- the two tests over lists: what fast_line and slow_line share
// ref, alt: the CN lists of the low-frequency test (ref is sorted away)
inline void low_stats(std::vector<double>& ref, const std::vector<double>& alt, bool del, svt_classify_line& r)
{
    r.n_ref = (uint32_t)ref.size();
    r.n_alt = (uint32_t)alt.size();
    if (!ref.empty()) {
        std::vector<uint64_t> keys(ref.size());
        for (size_t i = 0; i < ref.size(); ++i) keys[i] = key_of(ref[i]);
        std::sort(keys.begin(), keys.end());
        r.median = median_sorted(keys.data(), r.n_ref);
        for (uint64_t& k : keys) k = key_of(std::fabs(value_of(k) - r.median));
        std::sort(keys.begin(), keys.end());
        r.mad = median_sorted(keys.data(), r.n_ref);
        for (double cn : alt) r.quorum += supports(cn, r.median, r.mad, del);
    }
    finish_low(r);
}

// inc[s]: sample s enters the regression with x[s] (AB) and y[s] (CN, doubled for a male on X or Y)
inline void high_stats(const std::vector<uint8_t>& inc, const std::vector<double>& x, const std::vector<double>& y, bool has_cn, bool del,
                       const Params& pr, svt_classify_line& r)
{
    Tree sx, sy, sxx, syy, sxy;
    double x_lo = HUGE_VAL, x_hi = -HUGE_VAL, y_lo = HUGE_VAL, y_hi = -HUGE_VAL;
    uint32_t n = 0;
    for (uint32_t s = 0; s < inc.size(); ++s) {
        if (!inc[s]) continue;
        ++n;
        sx.add(s, x[s]);
        sy.add(s, y[s]);
        x_lo = std::min(x_lo, x[s]);
        x_hi = std::max(x_hi, x[s]);
        y_lo = std::min(y_lo, y[s]);
        y_hi = std::max(y_hi, y[s]);
    }
    r.n_regressed = n;
    const bool distinct = n > 0 && x_lo < x_hi && y_lo < y_hi;
    if (has_cn && distinct) {
        const double mx = sx.total() / (double)n, my = sy.total() / (double)n;
        for (uint32_t s = 0; s < inc.size(); ++s) {
            if (!inc[s]) continue;
            const double dx = x[s] - mx, dy = y[s] - my;
            sxx.add(s, dx * dx);
            syy.add(s, dy * dy);
            sxy.add(s, dx * dy);
        }
    }
    finish_high(r, has_cn, distinct, sxx.total(), syy.total(), sxy.total(), del, pr);
}

// where the sample columns of a line begin: starts[0 .. count), the columns behind the ninth tab
inline void column_starts(const uint8_t* p, const Head& h, std::vector<uint32_t>& starts)
{
    starts.clear();
    if (h.samples_b >= h.n) return;
    starts.push_back(h.samples_b);
    for (uint32_t i = h.samples_b; i < h.n; ++i)
        if (p[i] == '\t') starts.push_back(i + 1);
}

// The host twin of svt_classify_kernel for one line: its record, the marks the kernel would set included.  A marked line's
// values are slow_line's
inline svt_classify_line fast_line(const Block& b, const uint8_t* p, uint64_t len)
{
    Head h;
    scan_head(p, len, b.format_table, b.pr.format_len, h);
    if (!h.svtype) return empty_record(SVT_CLASSIFY_VERBATIM, 0);
    const uint32_t type = h.svtype == 1 ? SVT_CLASSIFY_DEL : 0u, n = b.pr.n_samples;
    if (h.slow) return empty_record(SVT_CLASSIFY_LOW, h.slow | type);
    if (!n || n > kCapacity) return empty_record(SVT_CLASSIFY_LOW, SVT_CLASSIFY_SLOW_CAPACITY | type);
    std::vector<uint32_t> starts;
    column_starts(p, h, starts);
    if (starts.size() != n) return empty_record(SVT_CLASSIFY_LOW, SVT_CLASSIFY_SLOW_COLUMNS | type);
    std::vector<Sample> sm(n);
    uint32_t slow = 0, n_pos = 0, male_alt = 0, female_alt = 0;
    for (uint32_t s = 0; s < n; ++s) {
        parse_sample(p, starts[s], s + 1 < n ? starts[s + 1] - 1 : h.n, h, sm[s]);
        slow |= sm[s].slow;
        if (h.sex && b.no_gender(s)) slow |= SVT_CLASSIFY_SLOW_GENDER;
        if (b.excluded[s]) continue;
        n_pos += sm[s].gt != kGtMissing && sm[s].gt != kGtRef;
        const bool alt = sm[s].gt == kGtHet || sm[s].gt == kGtHom;
        male_alt += alt && b.is_male(s);
        female_alt += alt && b.is_female(s);
    }
    svt_classify_line r = empty_record(n_pos < kMinPosForRegression ? SVT_CLASSIFY_LOW : SVT_CLASSIFY_HIGH, type);
    r.n_pos = n_pos;
    slow |= route_keys(r.route, h);
    if (slow) {
        r.flags |= slow;
        return r;
    }
    const bool del = h.svtype == 1;
    if (r.route == SVT_CLASSIFY_LOW) {
        const uint32_t pick = !h.sex ? 0u : male_alt > female_alt ? 1u : 2u;
        std::vector<double> ref, alt;
        for (uint32_t s = 0; s < n; ++s) {
            if (b.excluded[s]) continue;
            const uint32_t list = low_list(sm[s].gt, pick, b.is_male(s), b.is_female(s));
            if (list == 1) ref.push_back(sm[s].cn);
            if (list == 2) alt.push_back(sm[s].cn);
        }
        low_stats(ref, alt, del, r);
    } else {
        std::vector<uint8_t> inc(n);
        std::vector<double> x(n), y(n);
        for (uint32_t s = 0; s < n; ++s) {
            inc[s] = h.cn_i != kNone && sm[s].has_ab;   // (without CN in FORMAT the script looks at nothing)
            x[s] = sm[s].ab;
            y[s] = h.sex && b.is_male(s) ? sm[s].cn * 2.0 : sm[s].cn;
        }
        high_stats(inc, x, y, h.cn_i != kNone, del, b.pr, r);
    }
    return r;
}

// ---- the script's Variant in plain C++: what slow_line and the writer share
struct Variant {
    std::vector<std::pair<uint32_t, uint32_t>> col;            // the columns of the right-stripped line
    std::string chrom, pos, id, ref, alt, qual, filter;        // pos: str(int()); qual: '%0.2f'
    std::vector<std::pair<std::string, std::string>> info;     // a dict: a later key replaces an earlier one's value
    std::vector<uint8_t> active;                               // [header FORMAT id]
    std::vector<std::vector<std::string>> value;               // [sample][header FORMAT id]
    std::vector<std::vector<uint8_t>> has;

    const std::string* get_info(const std::string& key) const
    {
        for (const auto& kv : info)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
    void set_info(const std::string& key, const std::string& v)
    {
        for (auto& kv : info)
            if (kv.first == key) {
                kv.second = v;
                return;
            }
        info.emplace_back(key, v);
    }
    void del_info(const std::string& key)
    {
        for (size_t k = 0; k < info.size(); ++k)
            if (info[k].first == key) {
                info.erase(info.begin() + (long)k);
                return;
            }
    }
};

inline uint32_t format_index(const Block& b, const std::string& key)
{
    for (uint32_t k = 0; k < b.formats.size(); ++k)
        if (b.formats[k] == key) return k;
    return kNone;
}

inline std::string bytes(const uint8_t* p, uint32_t b, uint32_t e) { return std::string((const char*)p + b, e - b); }

inline void split(const uint8_t* p, uint32_t b, uint32_t e, uint8_t c, std::vector<std::pair<uint32_t, uint32_t>>& out)
{
    out.clear();
    for (uint32_t at = b; at <= e;) {
        uint32_t fe = at;
        while (fe < e && p[fe] != c) ++fe;
        out.emplace_back(at, fe);
        at = fe + 1;
    }
}

inline uint32_t stripped(const uint8_t* p, uint64_t len)
{
    uint32_t n = len > paste::kMaxLine ? paste::kMaxLine : (uint32_t)len;
    while (n && is_space(p[n - 1])) --n;
    return n;
}

// Variant(v, vcf) of the script, in its order; `samples`: the sample columns too (the writer of an unmarked line copies them)
inline bool parse_variant(const Block& b, const uint8_t* p, uint64_t len, bool samples, Variant& v, Bad& bad)
{
    const uint32_t n = stripped(p, len);
    split(p, 0, n, '\t', v.col);
    if (len > paste::kMaxLine || v.col.size() < 8) {
        bad.kind = SVT_CLASSIFY_BAD_COLUMNS;
        return false;
    }
    auto column = [&](size_t k) { return bytes(p, v.col[k].first, v.col[k].second); };
    v.chrom = column(0);
    if (!paste::py_int_text(p, v.col[1].first, v.col[1].second, v.pos)) {
        bad.kind = SVT_CLASSIFY_BAD_POS;
        bad.text = column(1);
        return false;
    }
    v.id = column(2);
    v.ref = column(3);
    v.alt = column(4);
    double q = 0.0;
    if (!bcf::is_dot(p, v.col[5].first, v.col[5].second) && !paste::py_float(p, v.col[5].first, v.col[5].second, q)) {
        bad.kind = SVT_CLASSIFY_BAD_QUAL;
        bad.text = column(5);
        return false;
    }
    v.qual = paste::fixed2(q);
    v.filter = column(6);
    v.active.assign(b.formats.size(), 0);
    v.value.clear();
    v.has.clear();
    if (samples) {
        std::vector<std::pair<uint32_t, uint32_t>> keys, fields;
        std::vector<uint32_t> key_index;
        static const uint8_t gt[] = "GT";
        if (v.col.size() < 9) keys.emplace_back(0, 2);
        else split(p, v.col[8].first, v.col[8].second, ':', keys);
        const uint8_t* kp = v.col.size() < 9 ? gt : p;
        for (const auto& k : keys) key_index.push_back(format_index(b, bytes(kp, k.first, k.second)));
        v.value.assign(b.pr.n_samples, std::vector<std::string>(b.formats.size()));
        v.has.assign(b.pr.n_samples, std::vector<uint8_t>(b.formats.size(), 0));
        for (uint32_t s = 0; s < b.pr.n_samples; ++s) {
            v.active[0] = v.has[s][0] = 1;
            if (9 + (size_t)s >= v.col.size()) {
                v.value[s][0] = "./.";
                continue;
            }
            split(p, v.col[9 + s].first, v.col[9 + s].second, ':', fields);
            v.value[s][0] = bytes(p, fields[0].first, fields[0].second);
            for (size_t j = 0; j < keys.size() && j < fields.size(); ++j) {
                if (key_index[j] == kNone) {
                    bad.kind = SVT_CLASSIFY_BAD_FORMAT;
                    bad.text = bytes(kp, keys[j].first, keys[j].second);
                    return false;
                }
                v.active[key_index[j]] = v.has[s][key_index[j]] = 1;
                v.value[s][key_index[j]] = bytes(p, fields[j].first, fields[j].second);
            }
        }
    }
    v.info.clear();
    std::vector<std::pair<uint32_t, uint32_t>> items, parts;
    split(p, v.col[7].first, v.col[7].second, ';', items);
    for (const auto& item : items) {
        split(p, item.first, item.second, '=', parts);
        v.set_info(bytes(p, parts[0].first, parts[0].second), parts.size() > 1 ? bytes(p, parts[1].first, parts[1].second) : std::string("True"));
    }
    return true;
}

// float(genotype.get_format(key)) of sample s
inline bool sample_float(const Block& b, const Variant& v, uint32_t s, const char* key, double& out, Bad& bad)
{
    const uint32_t k = format_index(b, key);
    bad.sample = s;
    if (k == kNone || !v.has[s][k]) {
        bad.kind = SVT_CLASSIFY_BAD_KEY;
        bad.text = key;
        return false;
    }
    const std::string& t = v.value[s][k];
    bad.text = t;
    if (!paste::py_float((const uint8_t*)t.data(), 0, (uint32_t)t.size(), out)) {
        bad.kind = SVT_CLASSIFY_BAD_NUMBER;
        return false;
    }
    if (!std::isfinite(out)) {
        bad.kind = SVT_CLASSIFY_BAD_NONFINITE;
        return false;
    }
    return true;
}

inline bool need_gender(const Block& b, uint32_t s, Bad& bad)
{
    if (!b.no_gender(s)) return true;
    bad.kind = SVT_CLASSIFY_BAD_GENDER;
    bad.sample = s;
    return false;
}

// The whole of one line in plain C++, as the script computes it, in the script's order: r (the marks kept), or `bad`
inline bool slow_line(const Block& b, const uint8_t* p, uint64_t len, svt_classify_line& r, Bad& bad)
{
    const uint32_t marks = r.flags & SVT_CLASSIFY_SLOW;
    bad = Bad();
    Head h;
    scan_head(p, len, b.format_table, b.pr.format_len, h);
    if (!h.svtype) {                                // (no marked line comes here: for a caller that has no rule)
        r = empty_record(SVT_CLASSIFY_VERBATIM, marks);
        return true;
    }
    Variant v;
    if (!parse_variant(b, p, len, true, v, bad)) return false;
    const std::string* type = v.get_info("SVTYPE");
    const bool del = type && *type == "DEL";
    if (!del && !(type && *type == "DUP")) {
        r = empty_record(SVT_CLASSIFY_DROPPED, marks);
        return true;
    }
    const uint32_t n = b.pr.n_samples;
    const bool sex = v.chrom == "X" || v.chrom == "Y";
    uint32_t n_pos = 0;
    for (uint32_t s = 0; s < n; ++s) n_pos += !b.excluded[s] && v.value[s][0] != "./." && v.value[s][0] != "0/0";
    r = empty_record(n_pos < kMinPosForRegression ? SVT_CLASSIFY_LOW : SVT_CLASSIFY_HIGH, marks | (del ? SVT_CLASSIFY_DEL : 0u));
    r.n_pos = n_pos;
    auto gt_class = [&](uint32_t s) {
        const std::string& g = v.value[s][0];
        return g == "0/0" ? kGtRef : g == "0/1" ? kGtHet : g == "1/1" ? kGtHom : kGtOther;
    };
    if (r.route == SVT_CLASSIFY_LOW) {
        std::vector<double> cn(n, 0.0);
        uint32_t male_alt = 0, female_alt = 0;
        for (uint32_t s = 0; s < n; ++s) {
            if (b.excluded[s]) continue;
            if (!sample_float(b, v, s, "CN", cn[s], bad)) return false;
            const uint32_t g = gt_class(s);
            if (sex && g != kGtOther && !need_gender(b, s, bad)) return false;
            male_alt += (g == kGtHet || g == kGtHom) && b.is_male(s);
            female_alt += (g == kGtHet || g == kGtHom) && b.is_female(s);
        }
        const uint32_t pick = !sex ? 0u : male_alt > female_alt ? 1u : 2u;
        std::vector<double> ref, alt;
        for (uint32_t s = 0; s < n; ++s) {
            if (b.excluded[s]) continue;
            const uint32_t list = low_list(gt_class(s), pick, b.is_male(s), b.is_female(s));
            if (list == 1) ref.push_back(cn[s]);
            if (list == 2) alt.push_back(cn[s]);
        }
        low_stats(ref, alt, del, r);
        return true;
    }
    const uint32_t cn_k = format_index(b, "CN"), ab_k = format_index(b, "AB");
    const bool has_cn = cn_k != kNone && v.active[cn_k];
    std::vector<uint8_t> inc(n, 0);
    std::vector<double> x(n, 0.0), y(n, 0.0);
    if (has_cn) {
        for (uint32_t s = 0; s < n; ++s) {
            if (ab_k != kNone && v.has[s][ab_k] && v.value[s][ab_k] == ".") continue;
            if (!sample_float(b, v, s, "AB", x[s], bad)) return false;
            inc[s] = x[s] != -1.0;
        }
        for (uint32_t s = 0; s < n; ++s) {
            if (sex && !need_gender(b, s, bad)) return false;
            if (!sample_float(b, v, s, "CN", y[s], bad)) return false;
            if (sex && b.is_male(s)) y[s] *= 2.0;
        }
    }
    high_stats(inc, x, y, has_cn, del, b.pr, r);
    return true;
}

// ---- the writer
// get_info_string: the header's order, a Flag by its id alone
inline std::string info_string(const Block& b, const Variant& v)
{
    std::string out;
    bool first = true;
    for (const auto& key : b.info) {
        const std::string* value = v.get_info(key.first);
        if (!value) continue;
        if (!first) out += ';';
        first = false;
        out += key.first;
        if (!key.second) {
            out += '=';
            out += *value;
        }
    }
    return out;
}

// get_var_string and its newline; `tail`: FORMAT and the sample columns
inline void var_string(const Block& b, const Variant& v, const std::string& tail, std::string& out)
{
    for (const std::string* f : {&v.chrom, &v.pos, &v.id, &v.ref, &v.alt, &v.qual, &v.filter}) {
        out += *f;
        out += '\t';
    }
    out += info_string(b, v);
    out += '\t';
    out += tail;
    out += '\n';
}

// FORMAT and the sample columns of a parsed line: the active keys in the header's order, "." where a sample lacks one
inline std::string generic_tail(const Block& b, const Variant& v)
{
    std::string out;
    bool first = true;
    for (size_t k = 0; k < b.formats.size(); ++k) {
        if (!v.active[k]) continue;
        if (!first) out += ':';
        first = false;
        out += b.formats[k];
    }
    out += '\t';
    for (uint32_t s = 0; s < b.pr.n_samples; ++s) {
        if (s) out += '\t';
        first = true;
        for (size_t k = 0; k < b.formats.size(); ++k) {
            if (!v.active[k]) continue;
            if (!first) out += ':';
            first = false;
            if (v.has[s][k]) out += v.value[s][k];
            else out += '.';
        }
    }
    return out;
}

// to_bnd: the two lines of an unsupported call, or the INFO key the line lacks
inline bool bnd_lines(const Block& b, const Variant& v, bool del, const std::string& tail, std::string& out, Bad& bad)
{
    const char* needed[] = {"END", "CIEND", "CIPOS", "CIEND95", "CIPOS95", "SVLEN"};
    for (const char* key : needed)
        if (!v.get_info(key)) {
            bad.kind = SVT_CLASSIFY_BAD_KEY;
            bad.text = key;
            return false;
        }
    const std::string end = *v.get_info("END");
    Variant v1 = v, v2 = v;
    for (Variant* m : {&v1, &v2}) {
        m->set_info("SVTYPE", "BND");
        m->set_info("EVENT", v.id);
    }
    v1.id = v.id + "_1";
    v2.id = v.id + "_2";
    v1.set_info("MATEID", v2.id);
    v2.set_info("MATEID", v1.id);
    v2.pos = end;
    v2.set_info("CIPOS", *v.get_info("CIEND"));
    v2.set_info("CIEND", *v.get_info("CIPOS"));
    v2.set_info("CIPOS95", *v.get_info("CIEND95"));
    v2.set_info("CIEND95", *v.get_info("CIPOS95"));
    for (Variant* m : {&v1, &v2}) {
        m->del_info("SVLEN");
        m->del_info("END");
    }
    v2.set_info("SECONDARY", "True");
    const std::string to_end = v.chrom + ":" + end, to_pos = v.chrom + ":" + v.pos;
    v1.alt = del ? "N[" + to_end + "[" : "]" + to_end + "]N";
    v2.alt = del ? "]" + to_pos + "]N" : "N[" + to_pos + "[";
    var_string(b, v1, tail, out);
    var_string(b, v2, tail, out);
    return true;
}

// what one line's record makes of it, appended to `out`
inline bool write_line(const Block& b, const uint8_t* p, uint64_t len, const svt_classify_line& r, std::string& out, Bad& bad)
{
    bad = Bad();
    if (r.route == SVT_CLASSIFY_VERBATIM) {
        out.append((const char*)p, len);
        return true;
    }
    if (r.route != SVT_CLASSIFY_LOW && r.route != SVT_CLASSIFY_HIGH) return true;
    const bool marked = (r.flags & SVT_CLASSIFY_SLOW) != 0;
    Variant v;
    if (!parse_variant(b, p, len, marked, v, bad)) return false;
    std::string tail;
    if (marked) tail = generic_tail(b, v);
    else if (v.col.size() > 8) tail = bytes(p, v.col[8].first, stripped(p, len));  // FORMAT in the header's order, every sample whole
    else {
        bad.kind = SVT_CLASSIFY_BAD_COLUMNS;        // (a record that is not this line's)
        return false;
    }
    if (r.verdict) {
        var_string(b, v, tail, out);
        return true;
    }
    return bnd_lines(b, v, (r.flags & SVT_CLASSIFY_DEL) != 0, tail, out, bad);
}

inline void report(svt_classify_info& info, uint64_t bad_line, const Bad& bad)
{
    info.bad_line = bad_line;
    info.bad_kind = bad.kind;
    info.bad_sample = bad.sample;
    std::memset(info.bad_text, 0, sizeof info.bad_text);
    std::memcpy(info.bad_text, bad.text.data(), std::min(bad.text.size(), sizeof info.bad_text - 1));
}

// the arguments of both entry points as a Block, `info` cleared; or what is wrong with them
inline const char* take_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                                  const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip,
                                  double slope_threshold, double rsquared_threshold, const svt_classify_line* results, const uint64_t* n_lines,
                                  svt_classify_info* info, Block& b)
{
    if (!info || !n_lines || !results || (len && !text) || !format_table || (n_samples && (!male || !female || !excluded))) return "null argument";
    *info = svt_classify_info();
    if (len > paste::kMaxLine) return "svt_vcf_classify: a block holds less than 2^31 bytes";
    if (format_len > 0xFFFFu || !parse_format_table(format_table, format_len, b.formats))
        return "svt_vcf_classify: format_table is \"<id>\\n\" per id, GT first";
    if (std::isnan(slope_threshold) || std::isnan(rsquared_threshold)) return "svt_vcf_classify: a threshold is a number";
    b.text = text;
    b.len = len;
    b.male = male;
    b.female = female;
    b.excluded = excluded;
    b.skip = skip;
    b.format_table = format_table;
    b.pr.slope_threshold = slope_threshold;
    b.pr.rsquared_threshold = rsquared_threshold;
    b.pr.n_samples = n_samples;
    b.pr.format_len = (uint32_t)format_len;
    return nullptr;
}

// What follows the rule on both engines: the marked lines settled by slow_line, the counts.  Returns the 1-based number of
// the first line the script dies on (with `bad`), else 0
inline uint64_t settle_block(const Block& b, svt_classify_line* results, svt_classify_info& info, Bad& bad)
{
    for (uint64_t j = 0; j < b.n_table; ++j) {
        svt_classify_line& r = results[j];
        if (b.skip && b.skip[j]) {
            r = empty_record(SVT_CLASSIFY_SKIPPED, 0);
            continue;
        }
        if (r.flags & SVT_CLASSIFY_SLOW) {
            if (!slow_line(b, b.text + b.lines[j].off, b.lines[j].len, r, bad)) return j + 1;
            ++info.host_lines;
        }
        info.near_lines += (r.flags & SVT_CLASSIFY_NEAR) != 0;
    }
    return 0;
}

inline const char* classify_host(Block& b, std::vector<svt_tbx_line>& table, svt_classify_line* results, uint64_t capacity, uint64_t* n_lines,
                                 svt_classify_info& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    b.lines = table.data();
    b.n_table = table.size();
    *n_lines = table.size();
    if (table.size() > capacity) return "svt_vcf_classify: capacity is below the number of lines";
    for (uint64_t j = 0; j < b.n_table; ++j)
        if (!(b.skip && b.skip[j])) results[j] = fast_line(b, b.text + table[j].off, table[j].len);
    Bad bad;
    if (const uint64_t bad_line = settle_block(b, results, info, bad)) report(info, bad_line, bad);
    return nullptr;
}

// the writer's entry: the block's output into `out`, out_off[0 .. n_lines]
inline const char* write_block(Block& b, std::vector<svt_tbx_line>& table, const svt_classify_line* results, uint64_t n_lines, uint64_t* out_off,
                               std::string& out, svt_classify_info& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    if (table.size() != n_lines) return "svt_vcf_classify_write: one record per line of the text";
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

}  // namespace classify
}  // namespace svt
#endif  // SVT_VCF_CLASSIFY_H

// svt_vcf_classify.h -- the read-depth classifier of DEL and DUP lines: the per-line rule, the host twin of the kernel, the plain
// C++ of the lines outside the rule's envelope and the writer of the output text (include/svtyper_reads.h:
// svt_classify_line).
//
// ONE piece of source for both places that run the rule, as svt_vcf_paste.h is: check_head, parse_sample, the order-preserving
// keys, supports, finish_low and finish_high are compiled for the host (fast_line, any C++17 compiler: this is where they are
// proven against goldens made from the reference's scripts/sv_classifier.py, and sanitised) and for the device
// (svt_vcf_classify_kernel.h, one workgroup per line, lanes over samples).  Every load is checked against the line's length.
// What a cohort line is to every rule (its tabs, POS, QUAL and FORMAT, the script's Variant, the drivers) is svt_vcf_cohort_line.h's.
//
// What the script does with a DEL or DUP line: it counts the samples not excluded whose GT is neither "./." nor "0/0"; below
// ten it compares the CN of the carriers with the median and the median absolute deviation of the "0/0" samples' CN; from ten
// on it regresses CN on AB.  A supported line is written again field by field, an unsupported one as two BND lines.
//
// The envelope of the rule: at least ten columns, the head as cohort::check_head wants it, one SVTYPE item, one column per sample
// of the header, every column with exactly FORMAT's fields, every CN and every AB that is not "." inside bcf::double_exact, 1 to
// kCapacity samples, on X and Y every sample with a gender, and the keys the route reads in FORMAT.  Anything else marks the
// line (SVT_CLASSIFY_SLOW_*): nothing is guessed, slow_line decides it in plain C++ with strtod and either computes the script's
// values or names its error.
//
// The order of the double-precision sums is part of the contract (slope and r2 are bit-identical between the engines): sample s
// adds into partial s % 256 in sample order, the 256 partials are joined per 64 by halving (p[l] += p[l + d], d = 32 .. 1) and
// the four results as (w0 + w1) + (w2 + w3): what 256 lanes, an xor butterfly per wavefront and one exchange through LDS give.
#ifndef SVT_VCF_CLASSIFY_H
#define SVT_VCF_CLASSIFY_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"
#include "svt_vcf_cohort_line.h"

namespace svt {
namespace classify {

constexpr uint32_t kCapacity = SVT_CLASSIFY_CAPACITY;
constexpr uint32_t kMinPosForRegression = 10;
constexpr uint32_t kGtMissing = 0, kGtRef = 1, kGtHet = 2, kGtHom = 3, kGtOther = 4;
constexpr uint32_t kCn = 0, kAb = 1;               // Head::key_at: where CN and AB stand in FORMAT
constexpr double kNearBand = 1e-9;

using cohort::bytes_are;
using cohort::kBlock;
using cohort::kNone;
using cohort::Tabs;

struct Params {
    double slope_threshold, rsquared_threshold;
    uint32_t n_samples, format_len;
};

// what the first nine columns of one right-stripped line give
struct Head : cohort::Head {
    uint32_t svtype;                                // of the first item "SVTYPE=": 0 neither, 1 DEL, 2 DUP
    uint32_t sex;                                   // CHROM is exactly X or Y
};

SVT_HD void check_head(const uint8_t* p, uint32_t n, bool too_long, const Tabs& t, const uint8_t* table, uint32_t table_len, Head& h)
{
    cohort::begin_head(n, t, h);
    h.svtype = h.sex = 0;
    if (too_long || t.count < 7) {                  // (the script's IndexError: slow_line names it)
        h.slow = SVT_CLASSIFY_SLOW_HEAD;
        h.svtype = 1;
        return;
    }
    // INFO: the first item that starts "SVTYPE=" decides; a second item of that key can change the type behind it
    uint32_t keyed = 0;
    bool found = false;
    const uint32_t info_e = t.tab[7];
    for (uint32_t b = t.tab[6] + 1; b <= info_e;) {
        uint32_t e = b, eq = kNone;
        for (; e < info_e && p[e] != ';'; ++e)
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
    if (keyed > 1 || t.count < 9) h.slow |= SVT_CLASSIFY_SLOW_HEAD;         // (the rule wants a tenth column)
    h.sex = t.tab[0] == 1 && (p[0] == 'X' || p[0] == 'Y');
    cohort::check_head(p, t, table, table_len, SVT_CLASSIFY_SLOW_HEAD, SVT_CLASSIFY_SLOW_FORMAT, "CNAB", 2, h);
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
    const uint32_t fields = cohort::walk_fields(p, b, e, ':', [&](uint32_t idx, uint32_t at, uint32_t fe) {
        if (idx == 0) {
            if (bytes_are(p, at, fe, "./.", 3)) s.gt = kGtMissing;
            else if (bytes_are(p, at, fe, "0/0", 3)) s.gt = kGtRef;
            else if (bytes_are(p, at, fe, "0/1", 3)) s.gt = kGtHet;
            else if (bytes_are(p, at, fe, "1/1", 3)) s.gt = kGtHom;
        } else if (idx == h.key_at[kCn]) {
            if (bcf::double_exact(p, at, fe, s.cn)) s.slow |= SVT_CLASSIFY_SLOW_TOKEN;
        } else if (idx == h.key_at[kAb]) {
            if (!bcf::is_dot(p, at, fe)) {
                if (bcf::double_exact(p, at, fe, s.ab)) s.slow |= SVT_CLASSIFY_SLOW_TOKEN;
                s.has_ab = s.ab != -1.0;
            }
        }
    });
    if (fields != h.n_fmt) s.slow |= SVT_CLASSIFY_SLOW_SAMPLE;
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
    if (route == SVT_CLASSIFY_LOW) return h.key_at[kCn] == kNone ? SVT_CLASSIFY_SLOW_KEYS : 0u;
    return h.key_at[kCn] != kNone && h.key_at[kAb] == kNone ? SVT_CLASSIFY_SLOW_KEYS : 0u;
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

using cohort::Bad;
using cohort::bytes;
using cohort::format_index;
using cohort::Variant;
using cohort::write_block;

// one block: cohort::Block with the per-sample tables, the lines that are not the rule's and the thresholds
struct Block : cohort::Block {
    static constexpr const char* kName = "svt_vcf_classify";
    static constexpr const char* kCapacityWhy = "svt_vcf_classify: capacity is below the number of lines";
    static constexpr const char* kWriteWhy = "svt_vcf_classify_write: one record per line of the text";
    static constexpr const char* kLengthWhy = "svt_vcf_classify: a block holds less than 2^31 bytes";
    static constexpr const char* kFormatWhy = "svt_vcf_classify: format_table is \"<id>\\n\" per id, GT first";
    const uint8_t *male = nullptr, *female = nullptr, *excluded = nullptr, *skip = nullptr;
    Params pr = Params();
    bool is_male(uint32_t s) const { return male[s] == 1; }
    bool is_female(uint32_t s) const { return female[s] == 1; }
    bool no_gender(uint32_t s) const { return male[s] == SVT_CLASSIFY_NO_GENDER; }
    bool skipped(uint64_t j) const { return skip && skip[j]; }
};

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

// The host twin of svt_classify_kernel for one line: its record, the marks the kernel would set included.  A marked line's
// values are slow_line's
inline svt_classify_line fast_line(const Block& b, const uint8_t* p, uint64_t len)
{
    const Head h = cohort::head_of<Head>(b, p, len);
    if (!h.svtype) return empty_record(SVT_CLASSIFY_VERBATIM, 0);
    const uint32_t type = h.svtype == 1 ? SVT_CLASSIFY_DEL : 0u, n = b.pr.n_samples;
    if (h.slow) return empty_record(SVT_CLASSIFY_LOW, h.slow | type);
    if (!n || n > kCapacity) return empty_record(SVT_CLASSIFY_LOW, SVT_CLASSIFY_SLOW_CAPACITY | type);
    std::vector<uint32_t> starts;
    cohort::column_starts(p, h, starts);
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
            inc[s] = h.key_at[kCn] != kNone && sm[s].has_ab;   // (without CN in FORMAT the script looks at nothing)
            x[s] = sm[s].ab;
            y[s] = h.sex && b.is_male(s) ? sm[s].cn * 2.0 : sm[s].cn;
        }
        high_stats(inc, x, y, h.key_at[kCn] != kNone, del, b.pr, r);
    }
    return r;
}

// ---- the script's order in plain C++ (cohort::parse_variant is the script's Variant)
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
    if (!cohort::py_float((const uint8_t*)t.data(), 0, (uint32_t)t.size(), out)) {
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
    if (!cohort::head_of<Head>(b, p, len).svtype) {               // (no marked line comes here: for a caller that has no rule)
        r = empty_record(SVT_CLASSIFY_VERBATIM, marks);
        return true;
    }
    Variant v;
    if (!cohort::parse_variant(b, b.pr.n_samples, p, len, true, false, v, bad)) return false;
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
    cohort::var_string(b, v1, tail, out);
    cohort::var_string(b, v2, tail, out);
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
    if (!cohort::parse_variant(b, b.pr.n_samples, p, len, marked, false, v, bad)) return false;
    std::string tail;
    if (marked) tail = cohort::generic_tail(b, v);
    else if (v.col.size() > 8) tail = bytes(p, v.col[8].first, cohort::stripped_length(p, len));  // FORMAT in the header's order, every sample whole
    else {
        bad.kind = SVT_CLASSIFY_BAD_COLUMNS;        // (a record that is not this line's)
        return false;
    }
    if (r.verdict) {
        cohort::var_string(b, v, tail, out);
        return true;
    }
    return bnd_lines(b, v, (r.flags & SVT_CLASSIFY_DEL) != 0, tail, out, bad);
}

// the arguments of both entry points as a Block, `info` cleared; or what is wrong with them
inline const char* take_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* male, const uint8_t* female,
                                  const uint8_t* excluded, const uint8_t* format_table, uint64_t format_len, const uint8_t* skip,
                                  double slope_threshold, double rsquared_threshold, const svt_classify_line* results, const uint64_t* n_lines,
                                  svt_classify_info* info, Block& b)
{
    if (const char* why = cohort::take_block_arguments(text, len, n_samples, format_table, format_len,
                                                       n_lines && results && (!n_samples || (male && female && excluded)), info, b))
        return why;
    if (std::isnan(slope_threshold) || std::isnan(rsquared_threshold)) return "svt_vcf_classify: a threshold is a number";
    b.male = male;
    b.female = female;
    b.excluded = excluded;
    b.skip = skip;
    b.pr.slope_threshold = slope_threshold;
    b.pr.rsquared_threshold = rsquared_threshold;
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
    return cohort::rule_host(b, table, results, capacity, n_lines, info);
}

}  // namespace classify
}  // namespace svt
#endif  // SVT_VCF_CLASSIFY_H

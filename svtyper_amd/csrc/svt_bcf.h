// svt_bcf.h -- VCF data lines as BCF2.2 records (VCFv4.3 specification, section 6): the record rule, the dictionaries it reads
// and the host twin of the kernels (include/svtyper_bcf.h).
//
// ONE piece of source for both places that run the rule, as svt_vcf_lines.h is: encode_line is compiled for the host
// (encode_host, any C++17 compiler: this is where it is proven against the independent reader of tests/bcfreader.py and
// sanitised) and for the device (svt_bcf_kernel.h, one lane per line).  It walks one line twice with the same code -- a Sink
// without a buffer counts, one with a buffer stores -- so the measuring pass and the writing pass cannot disagree; every load
// is checked against the line's length, every store against the sink's capacity; no std::, no allocation, no arrays.
//
// The dictionaries are flat tables (Dict: a view of pointers, host or device memory): the names side by side, a type per
// category and key, and an open-addressed table of FNV-1a hashes whose hits are confirmed by comparing the whole name.
//
// Floats.  A float is (float)strtod(token), htslib's rule.  float_exact computes that without strtod where one IEEE double
// operation gives it: at most 15 significant digits (an integer below 2^53) and a decimal exponent of magnitude at most 22
// once the fraction digits are folded in (10^22 is a double) -- a multiply or a divide of two exactly representable numbers is
// the correctly rounded double, which the cast rounds to float32.  Whatever else (more digits, larger exponents, nan, inf,
// hex, a token strtod would refuse) is outside that envelope: device code marks the line (Measure::host) and the host twin,
// which has strtod, encodes that record.
#ifndef SVT_BCF_H
#define SVT_BCF_H

#include <stdint.h>

#include "../../include/svtyper_bcf.h"
#include "svt_geometry_math.h"

namespace svt {
namespace bcf {

constexpr uint32_t kNoKey = 0xFFFFFFFFu;
constexpr uint32_t kTypeNone = 0, kTypeInt = 1, kTypeFloat = 2, kTypeFlag = 3, kTypeString = 4;     // Dict::types (Character is a String)
constexpr uint32_t kBtInt8 = 1, kBtInt16 = 2, kBtInt32 = 3, kBtFloat = 5, kBtChar = 7;              // the low nibble of a typed descriptor
constexpr uint32_t kFloatMissing = 0x7F800001u, kFloatEov = 0x7F800002u;
constexpr int64_t kInt32Floor = -2147483640ll;      // the eight values below it are the reserved ones
constexpr uint32_t kMaxLine = 0x7FFFFFFFu;

// The header's dictionaries as the rule reads them.  types[3 k + c]: the Type of key k as a FILTER (c = 0: 1 where declared),
// an INFO (1) or a FORMAT (2), kTypeNone where the header does not declare it there.  slots / cslots: index or -1
struct Dict {
    const uint8_t* names;
    const uint32_t* name_off;
    const uint8_t* types;
    const int32_t* slots;
    const uint8_t* cnames;
    const uint32_t* cname_off;
    const int32_t* cslots;
    uint32_t mask, n_keys, cmask, n_contigs, n_sample;
};

// what one line becomes: sizes, the span's fields, a refusal (kind: SVT_BCF_KIND_*, at: where in the line its key or token
// begins) and whether a float of it lies outside the device envelope
struct Measure {
    uint32_t l_shared, l_indiv, kind, at, host;
    int32_t tid;
    uint32_t beg, end;
};

// counts always; stores where it has a buffer and room
struct Sink {
    uint8_t* out;
    uint64_t cap, n;
    SVT_HD void put(uint32_t b)
    {
        if (out && n < cap) out[n] = (uint8_t)b;
        ++n;
    }
    SVT_HD void put16(uint32_t v) { put(v & 255); put(v >> 8 & 255); }
    SVT_HD void put32(uint32_t v) { put16(v & 0xFFFF); put16(v >> 16); }
};

SVT_HD uint32_t hash_bytes(const uint8_t* p, uint32_t b, uint32_t e)
{
    uint32_t h = 2166136261u;
    for (uint32_t i = b; i < e; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// the index of p[b, e) among the names, kNoKey where it is none of them
SVT_HD uint32_t lookup(const uint8_t* names, const uint32_t* name_off, const int32_t* slots, uint32_t mask, const uint8_t* p, uint32_t b, uint32_t e)
{
    for (uint32_t at = hash_bytes(p, b, e) & mask, tries = 0; tries <= mask; at = (at + 1) & mask, ++tries) {
        const int32_t k = slots[at];
        if (k < 0) return kNoKey;
        const uint32_t nb = name_off[k], ne = name_off[k + 1];
        if (ne - nb != e - b) continue;
        uint32_t i = 0;
        while (i < e - b && names[nb + i] == p[b + i]) ++i;
        if (i == e - b) return (uint32_t)k;
    }
    return kNoKey;
}

SVT_HD uint32_t find(const uint8_t* p, uint32_t at, uint32_t end, uint8_t c)
{
    while (at < end && p[at] != c) ++at;
    return at;
}

SVT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
SVT_HD bool is_dot(const uint8_t* p, uint32_t b, uint32_t e) { return e - b == 1 && p[b] == '.'; }
SVT_HD bool is_word(const uint8_t* p, uint32_t b, uint32_t e, char c0, char c1, char c2)
{
    return e - b == (c2 ? 3u : 2u) && p[b] == (uint8_t)c0 && p[b + 1] == (uint8_t)c1 && (!c2 || p[b + 2] == (uint8_t)c2);
}

// p[b, e) as an integer a BCF int32 can hold: a sign, one to ten digits, inside [kInt32Floor, 2^31 - 1]
SVT_HD bool parse_int(const uint8_t* p, uint32_t b, uint32_t e, int64_t& v)
{
    const bool neg = b < e && p[b] == '-';
    if (b < e && (p[b] == '-' || p[b] == '+')) ++b;
    if (b == e || e - b > 10) return false;
    int64_t x = 0;
    for (uint32_t i = b; i < e; ++i) {
        if (!is_digit(p[i])) return false;
        x = x * 10 + (p[i] - '0');
    }
    v = neg ? -x : x;
    return v >= kInt32Floor && v <= 2147483647ll;
}

// 0: v is strtod(p[b, e)), computed exactly; 2: outside the envelope (the header of this file)
SVT_HD uint32_t double_exact(const uint8_t* p, uint32_t b, uint32_t e, double& v)
{
    uint32_t i = b;
    const bool neg = i < e && p[i] == '-';
    if (i < e && (p[i] == '-' || p[i] == '+')) ++i;
    uint64_t m = 0;
    int32_t sig = 0, frac = 0, digits = 0;
    bool point = false;
    for (; i < e; ++i) {
        if (p[i] == '.' && !point) {
            point = true;
            continue;
        }
        if (!is_digit(p[i])) break;
        ++digits;
        if (point) ++frac;
        if (sig || p[i] != '0') {
            if (++sig > 15) return 2;
            m = m * 10 + (p[i] - '0');
        }
        if (digits > 64) return 2;
    }
    if (!digits) return 2;
    int32_t ex = 0;
    if (i < e && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        const bool eneg = i < e && p[i] == '-';
        if (i < e && (p[i] == '-' || p[i] == '+')) ++i;
        if (i == e || e - i > 4) return 2;
        for (; i < e; ++i) {
            if (!is_digit(p[i])) return 2;
            ex = ex * 10 + (p[i] - '0');
        }
        if (eneg) ex = -ex;
    }
    if (i != e) return 2;
    const int32_t e10 = ex - frac;
    if (e10 > 22 || e10 < -22) return 2;
    double p10 = 1.0;                               // exact: every power up to 10^22 is a double
    for (int32_t k = e10 < 0 ? -e10 : e10; k; --k) p10 *= 10.0;
    const double d = e10 < 0 ? (double)m / p10 : (double)m * p10;
    v = neg ? -d : d;
    return 0;
}

// 0: f is (float)strtod(p[b, e)), computed exactly; 2: outside the envelope
SVT_HD uint32_t float_exact(const uint8_t* p, uint32_t b, uint32_t e, float& f)
{
    double d = 0.0;
    if (const uint32_t rc = double_exact(p, b, e, d)) return rc;
    f = (float)d;
    return 0;
}

// 0 and f; 1: no float; 2: for the host twin to decide (device code, which has no strtod)
SVT_HD uint32_t parse_float(const uint8_t* p, uint32_t b, uint32_t e, bool exact, float& f, uint32_t& outside);

SVT_HD uint32_t float_bits(float f)
{
    union { float f; uint32_t u; } x;
    x.f = f;
    return x.u;
}

SVT_HD uint32_t int_type(int64_t lo, int64_t hi)
{
    if (lo >= -120 && hi <= 127) return kBtInt8;
    if (lo >= -32760 && hi <= 32767) return kBtInt16;
    return kBtInt32;
}

// one integer in width `type`; `special`: 0 a value, 1 missing, 2 end-of-vector
SVT_HD void put_int(Sink& s, uint32_t type, int64_t v, uint32_t special)
{
    if (type == kBtInt8) s.put(special ? 0x7Fu + special : (uint32_t)v & 255u);
    else if (type == kBtInt16) s.put16(special ? 0x7FFFu + special : (uint32_t)v & 0xFFFFu);
    else s.put32(special ? 0x7FFFFFFFu + special : (uint32_t)v);
}

// a typed integer scalar (a key, a count)
SVT_HD void put_scalar(Sink& s, int64_t v)
{
    const uint32_t t = int_type(v, v);
    s.put(1u << 4 | t);
    put_int(s, t, v, 0);
}

// a typed descriptor of n values of `type`
SVT_HD void put_size(Sink& s, uint64_t n, uint32_t type)
{
    if (n < 15) s.put((uint32_t)n << 4 | type);
    else {
        s.put(15u << 4 | type);
        put_scalar(s, (int64_t)n);
    }
}

SVT_HD void put_string(Sink& s, const uint8_t* p, uint32_t b, uint32_t e)
{
    put_size(s, e - b, kBtChar);
    for (uint32_t i = b; i < e; ++i) s.put(p[i]);
}

// the comma-separated integers of p[b, e) ('.': missing): how many, and the least and largest of those present
SVT_HD bool scan_ints(const uint8_t* p, uint32_t b, uint32_t e, uint32_t& count, int64_t& lo, int64_t& hi)
{
    count = 0;
    for (uint32_t at = b;; ) {
        const uint32_t t = find(p, at, e, ',');
        ++count;
        if (!is_dot(p, at, t)) {
            int64_t v;
            if (!parse_int(p, at, t, v)) return false;
            if (v < lo) lo = v;
            if (v > hi) hi = v;
        }
        if (t >= e) return true;
        at = t + 1;
    }
}

// scan_ints' tokens in width `type`, then end-of-vector up to `width` values
SVT_HD void put_ints(Sink& s, const uint8_t* p, uint32_t b, uint32_t e, uint32_t type, uint32_t width)
{
    uint32_t count = 0;
    for (uint32_t at = b;; ) {
        const uint32_t t = find(p, at, e, ',');
        int64_t v = 0;
        const bool dot = is_dot(p, at, t) || !parse_int(p, at, t, v);
        put_int(s, type, v, dot ? 1 : 0);
        ++count;
        if (t >= e) break;
        at = t + 1;
    }
    for (; count < width; ++count) put_int(s, type, 0, 2);
}

// the comma-separated floats of p[b, e): 0, or 1 where a token is none; `outside` is raised where one is left to the host
SVT_HD uint32_t scan_floats(const uint8_t* p, uint32_t b, uint32_t e, bool exact, uint32_t& count, uint32_t& outside)
{
    count = 0;
    for (uint32_t at = b;; ) {
        const uint32_t t = find(p, at, e, ',');
        ++count;
        float f;
        if (!is_dot(p, at, t) && parse_float(p, at, t, exact, f, outside) == 1) return 1;
        if (t >= e) return 0;
        at = t + 1;
    }
}

SVT_HD void put_floats(Sink& s, const uint8_t* p, uint32_t b, uint32_t e, bool exact, uint32_t width)
{
    uint32_t count = 0, outside = 0;
    for (uint32_t at = b;; ) {
        const uint32_t t = find(p, at, e, ',');
        float f = 0.0f;
        if (is_dot(p, at, t)) s.put32(kFloatMissing);
        else {
            parse_float(p, at, t, exact, f, outside);
            s.put32(float_bits(f));
        }
        ++count;
        if (t >= e) break;
        at = t + 1;
    }
    for (; count < width; ++count) s.put32(kFloatEov);
}

// a GT: alleles parted by '/' or '|'; (allele + 1) << 1 | phased, '.' the allele -1, the first allele never phased
SVT_HD bool scan_gt(const uint8_t* p, uint32_t b, uint32_t e, uint32_t& count, int64_t& lo, int64_t& hi, Sink* s, uint32_t type)
{
    count = 0;
    uint32_t phased = 0;
    for (uint32_t at = b;; ) {
        uint32_t t = at;
        while (t < e && p[t] != '/' && p[t] != '|') ++t;
        int64_t a = -1;
        if (!is_dot(p, at, t) && (t == at || p[at] == '-' || p[at] == '+' || !parse_int(p, at, t, a) || a > 0x3FFFFFFE)) return false;
        const int64_t v = (a + 1) << 1 | phased;
        if (v < lo) lo = v;
        if (v > hi) hi = v;
        if (s) put_int(*s, type, v, 0);
        ++count;
        if (t >= e) return true;
        phased = p[t] == '|';
        at = t + 1;
    }
}

// field k (from 0) of the sample p[b, e): false where the sample has fewer; `last`: no field stands behind it
SVT_HD bool sample_field(const uint8_t* p, uint32_t b, uint32_t e, uint32_t k, uint32_t& fb, uint32_t& fe, bool& last)
{
    uint32_t at = b;
    for (uint32_t i = 0; i < k; ++i) {
        at = find(p, at, e, ':');
        if (at >= e) return false;
        ++at;
    }
    fb = at;
    fe = find(p, at, e, ':');
    last = fe >= e;
    return true;
}

SVT_HD uint32_t refuse(Measure& m, uint32_t kind, uint32_t at)
{
    m.kind = kind;
    m.at = at;
    return kind;
}

// One FORMAT key over every sample: the typed key, one descriptor, n_sample x count values.  p[sb, n): the sample columns.
// Called with a counting sink or a storing one: the same walk
SVT_HD uint32_t encode_format_key(const Dict& d, const uint8_t* p, uint32_t n, uint32_t sb, uint32_t k, bool last_key, uint32_t key, uint32_t type, bool gt,
                                  uint32_t key_at, bool exact, Sink& s, Measure& m)
{
    // first walk: the longest vector, the integers' range
    uint32_t width = 0;
    int64_t lo = 0x7FFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFll;
    for (uint32_t at = sb; at <= n; ) {
        const uint32_t se = find(p, at, n, '\t');
        uint32_t fb = 0, fe = 0, count = 1;
        bool last = true;
        if (sample_field(p, at, se, k, fb, fe, last)) {
            if (last_key && !last) return refuse(m, SVT_BCF_KIND_FORMAT_VALUE, key_at);      // more fields than FORMAT has keys
            if (gt) {
                if (!scan_gt(p, fb, fe, count, lo, hi, nullptr, 0)) return refuse(m, SVT_BCF_KIND_FORMAT_VALUE, key_at);
            } else if (type == kTypeInt) {
                if (!scan_ints(p, fb, fe, count, lo, hi)) return refuse(m, SVT_BCF_KIND_FORMAT_VALUE, key_at);
            } else if (type == kTypeFloat) {
                if (scan_floats(p, fb, fe, exact, count, m.host)) return refuse(m, SVT_BCF_KIND_FORMAT_VALUE, key_at);
            } else count = fe - fb;
        } else if (gt) {
            lo = lo < 0 ? lo : 0;
            hi = hi > 0 ? hi : 0;
        }
        if (count > width) width = count;
        at = se + 1;
    }
    const bool ints = gt || type == kTypeInt;
    const uint32_t bt = ints ? (lo > hi ? kBtInt8 : int_type(lo, hi)) : type == kTypeFloat ? kBtFloat : kBtChar;
    put_scalar(s, key);
    put_size(s, width, bt);
    // second walk: the values, each sample's padded to the longest
    for (uint32_t at = sb; at <= n; ) {
        const uint32_t se = find(p, at, n, '\t');
        uint32_t fb = 0, fe = 0, count = 0;
        bool last = true;
        const bool have = sample_field(p, at, se, k, fb, fe, last);
        if (gt) {
            int64_t l = 0, h = 0;
            if (have) scan_gt(p, fb, fe, count, l, h, &s, bt);
            else {
                put_int(s, bt, 0, 0);
                count = 1;
            }
            for (; count < width; ++count) put_int(s, bt, 0, 2);
        } else if (type == kTypeInt) {
            if (have) put_ints(s, p, fb, fe, bt, width);
            else
                for (uint32_t c = 0; c < width; ++c) put_int(s, bt, 0, c ? 2 : 1);
        } else if (type == kTypeFloat) {
            if (have) put_floats(s, p, fb, fe, exact, width);
            else
                for (uint32_t c = 0; c < width; ++c) s.put32(c ? kFloatEov : kFloatMissing);
        } else {
            if (have)
                for (uint32_t i = fb; i < fe; ++i) s.put(p[i]);
            else s.put('.');
            for (uint32_t c = have ? fe - fb : 1; c < width; ++c) s.put(0);
        }
        at = se + 1;
    }
    return 0;
}

// The line p[0, len) (its newline included where it has one) as a BCF record into `s`.  With a counting sink (s.out null) m
// is filled: sizes, span fields, refusal, envelope mark; with a storing one m holds what the counting walk found and the
// record's l_shared and l_indiv are written from it.  `exact`: floats by float_exact first (the device's rule; the host twin
// then settles what it leaves).  Returns m.kind
SVT_HD uint32_t encode_line(const Dict& d, const uint8_t* p, uint64_t len, bool exact, Sink& s, Measure& m)
{
    const bool counting = s.out == nullptr;
    if (counting) {
        m.l_shared = m.l_indiv = m.kind = m.at = m.host = 0;
        m.tid = -1;
        m.beg = m.end = 0;
    }
    if (len > kMaxLine) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t n = (uint32_t)(len && p[len - 1] == '\n' ? len - 1 : len);
    // the columns
    const uint32_t chrom_e = find(p, 0, n, '\t');
    if (chrom_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t pos_b = chrom_e + 1, pos_e = find(p, pos_b, n, '\t');
    if (pos_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t id_b = pos_e + 1, id_e = find(p, id_b, n, '\t');
    if (id_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t ref_b = id_e + 1, ref_e = find(p, ref_b, n, '\t');
    if (ref_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t alt_b = ref_e + 1, alt_e = find(p, alt_b, n, '\t');
    if (alt_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t qual_b = alt_e + 1, qual_e = find(p, qual_b, n, '\t');
    if (qual_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t filt_b = qual_e + 1, filt_e = find(p, filt_b, n, '\t');
    if (filt_e >= n) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
    const uint32_t info_b = filt_e + 1, info_e = find(p, info_b, n, '\t');
    const bool has_fmt = info_e < n;
    const uint32_t fmt_b = has_fmt ? info_e + 1 : n, fmt_e = find(p, fmt_b, n, '\t');
    const uint32_t samp_b = fmt_e < n ? fmt_e + 1 : n;
    // CHROM, POS
    const uint32_t tid = lookup(d.cnames, d.cname_off, d.cslots, d.cmask, p, 0, chrom_e);
    if (tid == kNoKey) return refuse(m, SVT_BCF_KIND_CONTIG, 0);
    int64_t pos = 0;
    if (pos_e == pos_b || !is_digit(p[pos_b]) || !parse_int(p, pos_b, pos_e, pos) || pos >= 2147483647ll) return refuse(m, SVT_BCF_KIND_POS, pos_b);
    const int64_t pos0 = pos - 1;
    // the counts of the fixed part
    uint32_t n_allele = 1;
    if (!is_dot(p, alt_b, alt_e)) {
        ++n_allele;
        for (uint32_t i = alt_b; i < alt_e; ++i) n_allele += p[i] == ',';
    }
    uint32_t n_info = 0;
    int64_t rlen = ref_e - ref_b;
    if (!is_dot(p, info_b, info_e)) {
        const uint32_t end_key = lookup(d.names, d.name_off, d.slots, d.mask, (const uint8_t*)"END", 0, 3);
        const bool end_int = end_key != kNoKey && d.types[3 * end_key + 1] == kTypeInt;
        bool end_seen = false;
        for (uint32_t at = info_b; at < info_e; ) {
            const uint32_t t = find(p, at, info_e, ';');
            if (t > at) {
                ++n_info;
                if (end_int && !end_seen && t - at > 4 && p[at] == 'E' && p[at + 1] == 'N' && p[at + 2] == 'D' && p[at + 3] == '=') {
                    end_seen = true;                // the first END decides; one behind POS gives the record its length
                    int64_t v;
                    if (parse_int(p, at + 4, find(p, at + 4, t, ','), v) && v > pos0) rlen = v - pos0;
                }
            }
            at = t + 1;
        }
    }
    uint32_t n_fmt = 0, n_sample_cols = 0;
    if (has_fmt) {
        n_fmt = 1;
        for (uint32_t i = fmt_b; i < fmt_e; ++i) n_fmt += p[i] == ':';
        if (fmt_e < n) {
            n_sample_cols = 1;
            for (uint32_t i = samp_b; i < n; ++i) n_sample_cols += p[i] == '\t';
        }
        if (n_sample_cols == 0 || n_sample_cols != d.n_sample) return refuse(m, SVT_BCF_KIND_SAMPLES, fmt_b);
    }
    if (n_allele > 0xFFFF || n_info > 0xFFFF) return refuse(m, SVT_BCF_KIND_INFO_VALUE, info_b);
    if (n_fmt > 0xFF || d.n_sample > 0xFFFFFF) return refuse(m, SVT_BCF_KIND_FORMAT_KEY, fmt_b);
    float qual = 0.0f;
    uint32_t qual_bits = kFloatMissing;
    if (!is_dot(p, qual_b, qual_e)) {
        if (parse_float(p, qual_b, qual_e, exact, qual, m.host) == 1) return refuse(m, SVT_BCF_KIND_QUAL, qual_b);
        qual_bits = float_bits(qual);
    }
    if (counting) {
        m.tid = (int32_t)tid;
        m.beg = pos0 < 0 ? 0u : (uint32_t)pos0;
        const int64_t end = (pos0 < 0 ? 0 : pos0) + rlen;
        m.end = end > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)end;
    }
    // the fixed part
    s.put32(m.l_shared);
    s.put32(m.l_indiv);
    s.put32(tid);
    s.put32((uint32_t)(int32_t)pos0);
    s.put32((uint32_t)(int32_t)(rlen > 2147483647ll ? 2147483647ll : rlen));
    s.put32(qual_bits);
    s.put32(n_allele << 16 | n_info);
    s.put32(n_fmt << 24 | d.n_sample);
    // ID, the alleles, FILTER
    if (is_dot(p, id_b, id_e)) put_size(s, 0, kBtChar);
    else put_string(s, p, id_b, id_e);
    put_string(s, p, ref_b, ref_e);
    if (n_allele > 1)
        for (uint32_t at = alt_b;; ) {
            const uint32_t t = find(p, at, alt_e, ',');
            put_string(s, p, at, t);
            if (t >= alt_e) break;
            at = t + 1;
        }
    if (is_dot(p, filt_b, filt_e)) put_size(s, 0, 0);
    else {
        uint32_t count = 0;
        int64_t hi = 0;
        for (uint32_t at = filt_b;; ) {
            const uint32_t t = find(p, at, filt_e, ';');
            const uint32_t key = lookup(d.names, d.name_off, d.slots, d.mask, p, at, t);
            if (key == kNoKey || d.types[3 * key] == kTypeNone) return refuse(m, SVT_BCF_KIND_FILTER, at);
            ++count;
            if ((int64_t)key > hi) hi = key;
            if (t >= filt_e) break;
            at = t + 1;
        }
        const uint32_t bt = int_type(0, hi);
        put_size(s, count, bt);
        for (uint32_t at = filt_b;; ) {
            const uint32_t t = find(p, at, filt_e, ';');
            put_int(s, bt, lookup(d.names, d.name_off, d.slots, d.mask, p, at, t), 0);
            if (t >= filt_e) break;
            at = t + 1;
        }
    }
    // INFO
    if (n_info)
        for (uint32_t at = info_b; at < info_e; ) {
            const uint32_t t = find(p, at, info_e, ';');
            if (t > at) {
                const uint32_t eq = find(p, at, t, '=');
                const uint32_t key = lookup(d.names, d.name_off, d.slots, d.mask, p, at, eq);
                const uint32_t type = key == kNoKey ? kTypeNone : d.types[3 * key + 1];
                if (type == kTypeNone) return refuse(m, SVT_BCF_KIND_INFO_KEY, at);
                put_scalar(s, key);
                const uint32_t vb = eq + 1;
                if (eq >= t || type == kTypeFlag) s.put(0);
                else if (type == kTypeInt) {
                    uint32_t count = 0;
                    int64_t lo = 0x7FFFFFFFFFFFll, hi = -0x7FFFFFFFFFFFll;
                    if (!scan_ints(p, vb, t, count, lo, hi)) return refuse(m, SVT_BCF_KIND_INFO_VALUE, at);
                    const uint32_t bt = lo > hi ? kBtInt8 : int_type(lo, hi);
                    put_size(s, count, bt);
                    put_ints(s, p, vb, t, bt, count);
                } else if (type == kTypeFloat) {
                    uint32_t count = 0;
                    if (scan_floats(p, vb, t, exact, count, m.host)) return refuse(m, SVT_BCF_KIND_INFO_VALUE, at);
                    put_size(s, count, kBtFloat);
                    put_floats(s, p, vb, t, exact, count);
                } else put_string(s, p, vb, t);
            }
            at = t + 1;
        }
    const uint64_t shared_end = s.n;
    // FORMAT and the samples, key by key
    if (n_fmt) {
        uint32_t k = 0;
        for (uint32_t at = fmt_b;; ++k) {
            const uint32_t t = find(p, at, fmt_e, ':');
            const uint32_t key = lookup(d.names, d.name_off, d.slots, d.mask, p, at, t);
            const uint32_t type = key == kNoKey ? kTypeNone : d.types[3 * key + 2];
            if (type == kTypeNone) return refuse(m, SVT_BCF_KIND_FORMAT_KEY, at);
            if (encode_format_key(d, p, n, samp_b, k, t >= fmt_e, key, type, is_word(p, at, t, 'G', 'T', 0), at, exact, s, m)) return m.kind;
            if (t >= fmt_e) break;
            at = t + 1;
        }
    }
    if (counting) {
        if (s.n - 8 > 0xFFFFFFFFull) return refuse(m, SVT_BCF_KIND_COLUMNS, 0);
        m.l_shared = (uint32_t)(shared_end - 8);
        m.l_indiv = (uint32_t)(s.n - shared_end);
    }
    return 0;
}

SVT_HD uint64_t record_bytes(const Measure& m) { return m.kind ? 0 : 8ull + m.l_shared + m.l_indiv; }

}  // namespace bcf
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "svt_vcf_lines.h"

namespace svt {
namespace bcf {

#if !defined(__HIP_DEVICE_COMPILE__)
// (float)strtod(token), the whole token and nothing in front of it: 0 and f, or 1
inline uint32_t float_strtod(const uint8_t* p, uint32_t b, uint32_t e, float& f)
{
    char buf[128];
    if (b == e || e - b >= sizeof buf || p[b] == ' ' || (p[b] >= '\t' && p[b] <= '\r')) return 1;
    std::memcpy(buf, p + b, e - b);
    buf[e - b] = 0;
    if (std::strlen(buf) != e - b) return 1;
    char* stop = nullptr;
    const double d = std::strtod(buf, &stop);
    if (stop != buf + (e - b)) return 1;
    f = (float)d;
    return 0;
}
#endif

SVT_HD uint32_t parse_float(const uint8_t* p, uint32_t b, uint32_t e, bool exact, float& f, uint32_t& outside)
{
    if (exact && float_exact(p, b, e, f) == 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    outside = 1;
    f = 0.0f;
    return 2;
#else
    if (exact) outside = 1;
    return float_strtod(p, b, e, f);
#endif
}

// the header's dictionaries, made once per text: the storage behind a Dict
struct Tables {
    std::vector<uint8_t> names, types, cnames;
    std::vector<uint32_t> name_off{0}, cname_off{0};
    std::vector<int32_t> slots, cslots;
    std::vector<uint64_t> contig_len;
    uint32_t n_sample = 0;
    uint64_t header_len = 0;        // the '#' lines in front of the first data line
    uint64_t header_lines = 0;

    uint32_t n_keys() const { return (uint32_t)name_off.size() - 1; }
    uint32_t n_contigs() const { return (uint32_t)cname_off.size() - 1; }
    uint64_t l_ref_max() const
    {
        uint64_t most = 0;
        for (uint64_t l : contig_len) most = l > most ? l : most;
        return most;
    }
    Dict view() const
    {
        return Dict{names.data(), name_off.data(), types.data(), slots.data(), cnames.data(), cname_off.data(), cslots.data(),
                    (uint32_t)slots.size() - 1, n_keys(), (uint32_t)cslots.size() - 1, n_contigs(), n_sample};
    }
};

// the value of `field=` in a ##KIND=<...> line's brackets: at their start or behind a comma, outside quotes
inline bool header_field(const uint8_t* p, uint64_t b, uint64_t e, const char* field, std::string& value)
{
    const uint64_t fl = std::strlen(field);
    bool quoted = false;
    for (uint64_t i = b; i + fl < e; ++i) {
        if (p[i] == '"') quoted = !quoted;
        if (quoted || (i != b && p[i - 1] != ',') || std::memcmp(p + i, field, fl) != 0 || p[i + fl] != '=') continue;
        uint64_t v = i + fl + 1, t = v;
        while (t < e && p[t] != ',' && p[t] != '>' && p[t] != '\n') ++t;
        value.assign((const char*)p + v, t - v);
        return true;
    }
    return false;
}

inline void hash_table(const std::vector<uint8_t>& names, const std::vector<uint32_t>& off, std::vector<int32_t>& slots)
{
    uint32_t size = 8;
    while (size < 2 * off.size()) size <<= 1;
    slots.assign(size, -1);
    for (uint32_t k = 0; k + 1 < off.size(); ++k) {
        uint32_t at = hash_bytes(names.data(), off[k], off[k + 1]) & (size - 1);
        while (slots[at] >= 0) at = (at + 1) & (size - 1);
        slots[at] = (int32_t)k;
    }
}

// The dictionaries of text[0, len)'s header: PASS, then every ID of the ##FILTER, ##INFO and ##FORMAT lines in order of first
// appearance (an ID of two categories is one entry); the ##contig IDs in order.  null, or what is wrong with the header
inline const char* make_tables(const uint8_t* text, uint64_t len, Tables& t)
{
    t = Tables();
    std::unordered_map<std::string, uint32_t> keys, contigs;
    auto key_of = [&](const std::string& id) {
        auto it = keys.find(id);
        if (it != keys.end()) return it->second;
        const uint32_t k = (uint32_t)keys.size();
        keys.emplace(id, k);
        t.names.insert(t.names.end(), id.begin(), id.end());
        t.name_off.push_back((uint32_t)t.names.size());
        t.types.insert(t.types.end(), 3, (uint8_t)kTypeNone);
        return k;
    };
    t.types.reserve(64);
    t.types[3 * key_of("PASS")] = 1;
    bool chrom_line = false;
    uint64_t at = 0;
    std::string id, type;
    while (at < len && text[at] == '#') {
        const void* nl = std::memchr(text + at, '\n', len - at);
        const uint64_t end = nl ? (uint64_t)((const uint8_t*)nl - text) + 1 : len;
        const uint8_t* p = text + at;
        const uint64_t n = end - at;
        ++t.header_lines;
        if (chrom_line) return "a '#' line behind the #CHROM line";
        static const char* const kKinds[3] = {"##FILTER=<", "##INFO=<", "##FORMAT=<"};
        for (uint32_t c = 0; c < 3; ++c) {
            const uint64_t lead = std::strlen(kKinds[c]);
            if (n < lead || std::memcmp(p, kKinds[c], lead) != 0 || !header_field(p, lead, n, "ID", id)) continue;
            uint8_t code = 1;
            if (c) {
                if (!header_field(p, lead, n, "Type", type)) return "an ##INFO or ##FORMAT line without a Type";
                code = type == "Integer" ? kTypeInt : type == "Float" ? kTypeFloat : type == "Flag" ? kTypeFlag
                       : type == "String" || type == "Character" ? kTypeString : kTypeNone;
                if (code == kTypeNone || (c == 2 && code == kTypeFlag)) return "an ##INFO or ##FORMAT line with a Type that is none";
            }
            const uint32_t k = key_of(id);
            if (t.types[3 * k + c] == kTypeNone) t.types[3 * k + c] = code;
        }
        static const char kContig[] = "##contig=<";
        if (n >= sizeof kContig - 1 && std::memcmp(p, kContig, sizeof kContig - 1) == 0 && header_field(p, sizeof kContig - 1, n, "ID", id) &&
            contigs.emplace(id, (uint32_t)contigs.size()).second) {
            t.cnames.insert(t.cnames.end(), id.begin(), id.end());
            t.cname_off.push_back((uint32_t)t.cnames.size());
            t.contig_len.push_back(header_field(p, sizeof kContig - 1, n, "length", type) ? std::strtoull(type.c_str(), nullptr, 10) : 0);
        }
        if (n >= 6 && std::memcmp(p, "#CHROM", 6) == 0) {
            chrom_line = true;
            uint32_t tabs = 0;
            for (uint64_t i = 0; i < n; ++i) tabs += p[i] == '\t';
            t.n_sample = tabs > 8 ? tabs - 8 : 0;
        }
        at = end;
    }
    if (!chrom_line) return "the text has no #CHROM line";
    if (at && text[at - 1] != '\n') return "the #CHROM line has no newline";
    if (at + 1 >= (1ull << 32)) return "the header is longer than l_text can say";
    t.header_len = at;
    t.names.push_back(0);           // (never empty: data() of an empty vector may be null)
    t.cnames.push_back(0);
    hash_table(t.names, t.name_off, t.slots);
    hash_table(t.cnames, t.cname_off, t.cslots);
    return nullptr;
}

// magic, l_text, the header text, NUL
inline void stream_header(const uint8_t* text, const Tables& t, std::vector<uint8_t>& out)
{
    static const uint8_t kMagic[5] = {'B', 'C', 'F', 2, 2};
    out.assign(kMagic, kMagic + 5);
    const uint32_t l_text = (uint32_t)t.header_len + 1;
    for (uint32_t i = 0; i < 4; ++i) out.push_back((uint8_t)(l_text >> 8 * i));
    out.insert(out.end(), text, text + t.header_len);
    out.push_back(0);
}

// what an encoding call leaves for svt_bcf_take
struct Held {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets, starts;
    std::vector<svt_bam_span> spans;
    void clear()
    {
        std::vector<uint8_t>().swap(bytes);
        std::vector<uint64_t>().swap(offsets);
        std::vector<uint64_t>().swap(starts);
        std::vector<svt_bam_span>().swap(spans);
    }
};

// The plan both routes share: the line table's body in the order written (perm, with `sort` the stable (contig rank, POS)
// order of tbx::sort_order).  0, or the 1-based number of a body line that is no data line
inline uint64_t body_order(const uint8_t* text, const std::vector<svt_tbx_line>& lines, const Tables& t, bool sort, std::vector<uint64_t>& order)
{
    const uint64_t n = lines.size(), h = t.header_lines;
    order.clear();
    if (sort) {
        std::vector<uint64_t> perm(n);
        if (const uint64_t bad = tbx::sort_order(text, lines.data(), n, perm.data())) return bad;
        order.assign(perm.begin() + (std::ptrdiff_t)h, perm.end());
    } else
        for (uint64_t i = h; i < n; ++i) order.push_back(i);
    return 0;
}

// a body line the order could not place (no data line by the line table's rule): refused in the record rule's own words
inline void refuse_unsortable(const Dict& d, const uint8_t* text, const std::vector<svt_tbx_line>& lines, uint64_t bad, svt_bcf_info& info)
{
    Sink count{nullptr, 0, 0};
    Measure m;
    const uint32_t kind = encode_line(d, text + lines[bad - 1].off, lines[bad - 1].len, false, count, m);
    info.bad_line = bad;
    info.bad_kind = kind ? kind : SVT_BCF_KIND_COLUMNS;
    info.bad_at = kind ? m.at : 0;
}

// the measures of the lines in written order -> the first refusal by line number, or the offsets and the spans
inline bool place_records(const std::vector<Measure>& m, const std::vector<uint64_t>& order, uint64_t base, svt_bcf_info& info, Held& held)
{
    uint64_t bad = 0;
    for (uint64_t j = 0; j < m.size(); ++j)
        if (m[j].kind && (!bad || order[j] + 1 < info.bad_line)) {
            bad = info.bad_line = order[j] + 1;
            info.bad_kind = m[j].kind;
            info.bad_at = m[j].at;
        }
    if (bad) return false;
    held.offsets.resize(m.size() + 1);
    held.spans.resize(m.size());
    uint64_t at = base;
    for (uint64_t j = 0; j < m.size(); ++j) {
        held.offsets[j] = at;
        const uint64_t size = record_bytes(m[j]);
        held.spans[j] = svt_bam_span{at, size, (uint64_t)(uint32_t)m[j].tid << 32 | m[j].beg, m[j].tid, m[j].beg, m[j].end, 0};
        at += size;
    }
    held.offsets[m.size()] = at;
    return true;
}

// svt_bcf_encode_host without its argument checks: the stream (header and records) into held.bytes.  `exact`: floats by the
// device's rule first; info.host_lines counts the lines it left to strtod
inline const char* encode_host(const uint8_t* text, uint64_t len, bool sort, bool exact, svt_bcf_info& info, Held& held)
{
    Tables t;
    if (const char* why = make_tables(text, len, t)) return why;
    const Dict d = t.view();
    std::vector<svt_tbx_line> lines(tbx::count_lines(text, len));
    tbx::lines_host(text, len, lines.data());
    info.n_ref = (int32_t)t.n_contigs();
    info.l_ref_max = t.l_ref_max();
    info.n_sample = t.n_sample;
    std::vector<uint64_t> order;
    if (const uint64_t bad = body_order(text, lines, t, sort, order)) {
        refuse_unsortable(d, text, lines, bad, info);
        return nullptr;
    }
    std::vector<Measure> m(order.size());
    for (uint64_t j = 0; j < order.size(); ++j) {
        Sink count{nullptr, 0, 0};
        encode_line(d, text + lines[order[j]].off, lines[order[j]].len, exact, count, m[j]);
        info.host_lines += m[j].host;
    }
    stream_header(text, t, held.bytes);
    info.header_len = held.bytes.size();
    if (!place_records(m, order, info.header_len, info, held)) return nullptr;
    held.bytes.resize(held.offsets.back());
    for (uint64_t j = 0; j < order.size(); ++j) {
        Sink store{held.bytes.data() + held.offsets[j], held.offsets[j + 1] - held.offsets[j], 0};
        encode_line(d, text + lines[order[j]].off, lines[order[j]].len, exact, store, m[j]);
        if (store.n != store.cap) return "svt_bcf_encode: a record's two walks disagree";
    }
    info.n_records = order.size();
    return nullptr;
}

}  // namespace bcf
}  // namespace svt
#endif  // SVT_BCF_H

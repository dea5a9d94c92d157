// svt_bcf_text.h -- BCF2.2 records back to VCF data lines (VCFv4.3 specification, section 6): the record rule, the dictionaries
// it reads and the host twin of the kernels (include/svtyper_bcf.h).  The inverse of svt_bcf.h.
//
// ONE piece of source for both places that run the rule, as svt_bcf.h is: shared_text and sample_text are compiled for the
// host (text_host, any C++17 compiler: this is where the rule is proven against tests/bcftext.py over the independent reader
// and sanitised) and for the device (svt_bcf_text_kernel.h, one wavefront per record, lanes over samples).  One walk serves
// both passes -- a Sink without a buffer counts, one with a buffer stores -- so the measuring pass and the writing pass
// cannot disagree; every load is checked against the record's l_shared / l_indiv, every store against the sink's capacity;
// the walk keeps no array.
//
// A record's line is two pieces.  shared_text walks the shared part (CHROM through INFO), then the individual part's
// descriptors -- per FORMAT key a typed key and one descriptor in front of n_sample x count values -- and writes the first
// eight columns and the FORMAT column; everything a record can be refused for is found there.  sample_text writes the
// column of ONE sample: it walks the same descriptors, and a key's block being n_sample * count * width bytes, the sample's
// values lie at an O(1) place per key.  The host twin calls it sample after sample; the kernels give every lane its samples.
//
// The dictionaries are flat tables (TextDict: a view of pointers, host or device memory): index -> name and a Type per
// category, contig index -> name.  IDX= is honoured where a header line carries it (sparse indices are legal: an index
// without a line is one the dictionaries do not hold); without it the order is the implicit one svt_bcf.h writes.
//
// Floats.  C's %g of the float widened to double.  float_text computes it exactly in integer arithmetic inside the
// envelope  x == 0 (either sign)  or  1e-4 <= |x| < 1e6:  there a float is m / 2^k with m < 2^24 and 4 <= k <= 37, the
// decimal exponent X lies in [-4, 5], and m * 10^(5 - X) is below 2^54 -- one 64-bit product whose low k bits are the
// remainder that round-half-even looks at (the six digits 999999.5 and up carry into "1e+06").  Whatever else (smaller,
// larger, subnormal, nan, inf) is outside: device code marks the record and the host twin, which has snprintf, writes it.
#ifndef SVT_BCF_TEXT_H
#define SVT_BCF_TEXT_H

#include "svt_bcf.h"

namespace svt {
namespace bcftext {

using bcf::Sink;
using bcf::kBtChar;
using bcf::kBtFloat;
using bcf::kBtInt16;
using bcf::kBtInt32;
using bcf::kBtInt8;
using bcf::kFloatEov;
using bcf::kFloatMissing;
using bcf::kNoKey;

// index -> name (names[name_off[k], name_off[k + 1])) and types[3 k + c], the Type of index k as a FILTER (c = 0: 1 where
// declared), an INFO (1) or a FORMAT (2), bcf::kTypeNone where the header does not hold it there; contig index -> name,
// chave[k]: whether a ##contig line holds index k.  gt_key: the index of "GT", or kNoKey
struct TextDict {
    const uint8_t* names;
    const uint32_t* name_off;
    const uint8_t* types;
    const uint8_t* cnames;
    const uint32_t* cname_off;
    const uint8_t* chave;
    uint32_t n_keys, n_contigs, n_sample, gt_key;
};

// what shared_text finds in a record besides its text
struct Shape {
    uint32_t l_shared, l_indiv, n_fmt, n_sample, kind, outside;
};

SVT_HD uint32_t load8(const uint8_t* p, uint32_t n, uint32_t at) { return at < n ? p[at] : 0u; }
SVT_HD uint32_t load16(const uint8_t* p, uint32_t n, uint32_t at) { return load8(p, n, at) | load8(p, n, at + 1) << 8; }
SVT_HD uint32_t load32(const uint8_t* p, uint32_t n, uint32_t at) { return load16(p, n, at) | load16(p, n, at + 2) << 16; }

SVT_HD uint32_t width_of(uint32_t type) { return type == kBtInt16 ? 2u : type == kBtInt32 || type == kBtFloat ? 4u : type == 0 ? 0u : 1u; }
SVT_HD bool is_int(uint32_t type) { return type >= kBtInt8 && type <= kBtInt32; }

// the integer of width `type` at p[at] (inside p[0, n) by the caller's check of the vector), sign-extended
SVT_HD int32_t load_int(const uint8_t* p, uint32_t n, uint32_t at, uint32_t type)
{
    if (type == kBtInt8) return (int32_t)(int8_t)load8(p, n, at);
    if (type == kBtInt16) return (int32_t)(int16_t)load16(p, n, at);
    return (int32_t)load32(p, n, at);
}
SVT_HD int32_t int_missing(uint32_t type) { return type == kBtInt8 ? -128 : type == kBtInt16 ? -32768 : (int32_t)0x80000000u; }
SVT_HD int32_t int_eov(uint32_t type) { return int_missing(type) + 1; }

// A typed descriptor at p[at]: its type and count, `at` moved behind it.  0, or the kind it is refused for
SVT_HD uint32_t read_descriptor(const uint8_t* p, uint32_t n, uint32_t& at, uint32_t& type, uint32_t& count)
{
    if (at >= n) return SVT_BCF_TEXT_KIND_LENGTH;
    const uint32_t b = p[at++];
    type = b & 15u;
    count = b >> 4;
    if (type != 0 && !is_int(type) && type != kBtFloat && type != kBtChar) return SVT_BCF_TEXT_KIND_TYPE;
    if (count == 15) {
        if (at >= n) return SVT_BCF_TEXT_KIND_COUNT;
        const uint32_t d = p[at++], t2 = d & 15u;
        if (d >> 4 != 1 || !is_int(t2) || n - at < width_of(t2)) return SVT_BCF_TEXT_KIND_COUNT;
        const int32_t v = load_int(p, n, at, t2);
        at += width_of(t2);
        if (v < 0) return SVT_BCF_TEXT_KIND_COUNT;
        count = (uint32_t)v;
    }
    return 0;
}

// descriptor and a check that its `times` x count values lie inside p[0, n); `at` is left at the first value
SVT_HD uint32_t read_vector(const uint8_t* p, uint32_t n, uint32_t& at, uint32_t& type, uint32_t& count, uint64_t times)
{
    if (const uint32_t kind = read_descriptor(p, n, at, type, count)) return kind;
    if (times * count * width_of(type) > (uint64_t)(n - at)) return SVT_BCF_TEXT_KIND_COUNT;
    return 0;
}

// a typed integer scalar (a dictionary index)
SVT_HD uint32_t read_key(const uint8_t* p, uint32_t n, uint32_t& at, uint32_t& key)
{
    uint32_t type = 0, count = 0;
    if (const uint32_t kind = read_vector(p, n, at, type, count, 1)) return kind;
    if (!is_int(type) || count != 1) return SVT_BCF_TEXT_KIND_TYPE;
    const int32_t v = load_int(p, n, at, type);
    at += width_of(type);
    key = v < 0 ? kNoKey : (uint32_t)v;
    return 0;
}

SVT_HD void put_bytes(Sink& s, const uint8_t* p, uint32_t b, uint32_t e)
{
    for (uint32_t i = b; i < e; ++i) s.put(p[i]);
}

SVT_HD void put_unsigned(Sink& s, uint64_t v)
{
    uint64_t div = 1;
    while (v / div >= 10) div *= 10;
    for (; div; div /= 10) s.put('0' + (uint32_t)(v / div % 10));
}

SVT_HD void put_signed(Sink& s, int64_t v)
{
    if (v < 0) s.put('-');
    put_unsigned(s, v < 0 ? (uint64_t)(-v) : (uint64_t)v);
}

// %g of the float with these bits where the envelope (the header of this file) holds it: true and its text, or false
SVT_HD bool float_exact_text(uint32_t bits, Sink& s)
{
    const uint32_t biased = bits >> 23 & 255u, frac = bits & 0x7FFFFFu;
    if ((bits & 0x7FFFFFFFu) == 0) {
        if (bits >> 31) s.put('-');
        s.put('0');
        return true;
    }
    if (biased < 150 - 37 || biased > 150 - 4) return false;
    const uint64_t m = frac | 0x800000u;
    const uint32_t k = 150 - biased;                // |x| = m / 2^k, 4 <= k <= 37
    if (m * 10000u < 1ull << k) return false;       // below 1e-4
    if (k == 4 && m >= 16000000u) return false;     // 1e6 and above
    // X: 10^X <= |x| < 10^(X + 1)
    int32_t X = 5;
    uint64_t up = 100000;                           // 10^X for X > 0, 10^-X below
    while (X > 0 && m < up << k) {
        --X;
        up /= 10;
    }
    if (X == 0) {
        up = 1;
        while (X > -4 && m * up < 1ull << k) {
            --X;
            up *= 10;
        }
    }
    uint64_t scale = 1;                             // 10^(5 - X): at most 10^9
    for (int32_t i = 5 - X; i > 0; --i) scale *= 10;
    const uint64_t N = m * scale, half = 1ull << (k - 1), rem = N & ((1ull << k) - 1);
    uint64_t q = N >> k;                            // six digits
    if (rem > half || (rem == half && (q & 1))) ++q;
    if (q == 1000000) {
        q = 100000;
        ++X;
    }
    if (bits >> 31) s.put('-');
    if (X == 6) {                                   // (999999.5 and up: the one exponent form inside the envelope)
        put_bytes(s, (const uint8_t*)"1e+06", 0, 5);
        return true;
    }
    uint32_t digits = 6;
    while (digits > 1 && q % 10 == 0) {
        q /= 10;
        --digits;
    }
    uint64_t div = 1;
    for (uint32_t i = 1; i < digits; ++i) div *= 10;
    if (X < 0) {
        s.put('0');
        s.put('.');
        for (int32_t i = -X - 1; i > 0; --i) s.put('0');
    }
    for (uint32_t i = 0; i < digits; ++i, div /= 10) {
        if (X >= 0 && i == (uint32_t)X + 1) s.put('.');
        s.put('0' + (uint32_t)(q / div % 10));
    }
    for (int32_t i = (int32_t)digits; X >= 0 && i < X + 1; ++i) s.put('0');
    return true;
}

// one float that is neither reserved pattern; `exact`: by float_exact_text first.  `outside` is raised where that leaves
// the float to the host (device code, which has no snprintf, then writes nothing: the host twin writes the record)
SVT_HD void put_float(Sink& s, uint32_t bits, bool exact, uint32_t& outside);

// a vector of `count` values of `type` at p[at], inside p[0, n) by the caller's check: INFO's and FORMAT's numeric rule
SVT_HD void put_numbers(Sink& s, const uint8_t* p, uint32_t n, uint32_t at, uint32_t type, uint32_t count, bool exact, uint32_t& outside)
{
    bool any = false;
    for (uint32_t i = 0; i < count; ++i) {
        if (type == kBtFloat) {
            const uint32_t bits = load32(p, n, at + 4 * i);
            if (bits == kFloatEov) break;
            if (any) s.put(',');
            if (bits == kFloatMissing) s.put('.');
            else put_float(s, bits, exact, outside);
        } else {
            const int32_t v = load_int(p, n, at + i * width_of(type), type);
            if (v == int_eov(type)) break;
            if (any) s.put(',');
            if (v == int_missing(type)) s.put('.');
            else put_signed(s, v);
        }
        any = true;
    }
    if (!any) s.put('.');
}

SVT_HD void put_gt(Sink& s, const uint8_t* p, uint32_t n, uint32_t at, uint32_t type, uint32_t count)
{
    bool any = false;
    for (uint32_t i = 0; i < count; ++i) {
        const int32_t v = load_int(p, n, at + i * width_of(type), type);
        if (v == int_eov(type)) break;
        if (any) s.put(v & 1 ? '|' : '/');
        if (v >> 1 == 0) s.put('.');
        else put_signed(s, (int64_t)(v >> 1) - 1);
        any = true;
    }
    if (!any) s.put('.');
}

SVT_HD bool put_name(Sink& s, const TextDict& d, uint32_t key, uint32_t category)
{
    if (key >= d.n_keys || d.types[3 * key + category] == bcf::kTypeNone) return false;
    put_bytes(s, d.names, d.name_off[key], d.name_off[key + 1]);
    return true;
}

SVT_HD uint32_t refuse(Shape& sh, uint32_t kind)
{
    sh.kind = kind;
    return kind;
}

// The record rec[0, len) -- l_shared, l_indiv, the shared part, the individual part -- checked from end to end, and its line
// up to and including the FORMAT column (no tab behind it, no newline) into `s`.  Returns sh.kind: 0, or what it is refused for
SVT_HD uint32_t shared_text(const TextDict& d, const uint8_t* rec, uint64_t len, bool exact, Sink& s, Shape& sh)
{
    sh.l_shared = sh.l_indiv = sh.n_fmt = sh.n_sample = sh.kind = sh.outside = 0;
    if (len < 8 || len > 0xFFFFFFFFull) return refuse(sh, SVT_BCF_TEXT_KIND_TRUNCATED);
    const uint32_t ls = load32(rec, 8, 0), li = load32(rec, 8, 4);
    if (ls < 24 || 8ull + ls + li != len) return refuse(sh, SVT_BCF_TEXT_KIND_TRUNCATED);
    const uint8_t* p = rec + 8;
    const uint32_t tid = load32(p, ls, 0), pos0 = load32(p, ls, 4), qual = load32(p, ls, 12), nai = load32(p, ls, 16), nfs = load32(p, ls, 20);
    const uint32_t n_allele = nai >> 16, n_info = nai & 0xFFFFu, n_fmt = nfs >> 24, n_sample = nfs & 0xFFFFFFu;
    sh.l_shared = ls;
    sh.l_indiv = li;
    sh.n_fmt = n_fmt;
    sh.n_sample = n_sample;
    if (tid >= d.n_contigs || !d.chave[tid]) return refuse(sh, SVT_BCF_TEXT_KIND_INDEX);
    if (n_sample != d.n_sample) return refuse(sh, SVT_BCF_TEXT_KIND_SAMPLES);
    put_bytes(s, d.cnames, d.cname_off[tid], d.cname_off[tid + 1]);
    s.put('\t');
    put_signed(s, (int64_t)(int32_t)pos0 + 1);
    s.put('\t');
    // ID, the alleles
    uint32_t at = 24, type = 0, count = 0;
    if (const uint32_t kind = read_vector(p, ls, at, type, count, 1)) return refuse(sh, kind);
    if (type != kBtChar && type != 0) return refuse(sh, SVT_BCF_TEXT_KIND_TYPE);
    if (count == 0 || type == 0) s.put('.');
    else put_bytes(s, p, at, at + count);
    at += count * width_of(type);
    s.put('\t');
    for (uint32_t a = 0; a < n_allele; ++a) {
        if (const uint32_t kind = read_vector(p, ls, at, type, count, 1)) return refuse(sh, kind);
        if (type != kBtChar && type != 0) return refuse(sh, SVT_BCF_TEXT_KIND_TYPE);
        if (a == 1) s.put('\t');
        if (a > 1) s.put(',');
        put_bytes(s, p, at, at + count * width_of(type));
        at += count * width_of(type);
    }
    if (n_allele == 0) s.put('.');
    if (n_allele < 2) {
        s.put('\t');
        s.put('.');
    }
    s.put('\t');
    if (qual == kFloatMissing) s.put('.');
    else put_float(s, qual, exact, sh.outside);
    s.put('\t');
    // FILTER
    if (const uint32_t kind = read_vector(p, ls, at, type, count, 1)) return refuse(sh, kind);
    if (type == 0 || count == 0) s.put('.');
    else {
        if (!is_int(type)) return refuse(sh, SVT_BCF_TEXT_KIND_TYPE);
        for (uint32_t i = 0; i < count; ++i) {
            const int32_t v = load_int(p, ls, at + i * width_of(type), type);
            if (i) s.put(';');
            if (v < 0 || !put_name(s, d, (uint32_t)v, 0)) return refuse(sh, SVT_BCF_TEXT_KIND_INDEX);
        }
    }
    at += count * width_of(type);
    s.put('\t');
    // INFO
    if (n_info == 0) s.put('.');
    for (uint32_t i = 0; i < n_info; ++i) {
        uint32_t key = 0;
        if (const uint32_t kind = read_key(p, ls, at, key)) return refuse(sh, kind);
        if (i) s.put(';');
        if (!put_name(s, d, key, 1)) return refuse(sh, SVT_BCF_TEXT_KIND_INDEX);
        if (const uint32_t kind = read_vector(p, ls, at, type, count, 1)) return refuse(sh, kind);
        if (type != 0) {
            s.put('=');
            if (type == kBtChar) put_bytes(s, p, at, at + count);
            else put_numbers(s, p, ls, at, type, count, exact, sh.outside);
        }
        at += count * width_of(type);
    }
    if (at != ls) return refuse(sh, SVT_BCF_TEXT_KIND_LENGTH);
    // FORMAT: the keys; the blocks are checked here and read by sample_text
    const uint8_t* q = p + ls;
    at = 0;
    for (uint32_t k = 0; k < n_fmt; ++k) {
        uint32_t key = 0;
        if (const uint32_t kind = read_key(q, li, at, key)) return refuse(sh, kind);
        s.put(k ? ':' : '\t');
        if (!put_name(s, d, key, 2)) return refuse(sh, SVT_BCF_TEXT_KIND_INDEX);
        if (const uint32_t kind = read_vector(q, li, at, type, count, n_sample)) return refuse(sh, kind);
        if (key == d.gt_key && !is_int(type)) return refuse(sh, SVT_BCF_TEXT_KIND_GT);
        at += (uint32_t)((uint64_t)n_sample * count * width_of(type));
    }
    if (at != li) return refuse(sh, SVT_BCF_TEXT_KIND_LENGTH);
    return 0;
}

// The column of sample `sample` of a record shared_text accepted (sh: what it found), the tab in front of it included
SVT_HD void sample_text(const TextDict& d, const uint8_t* rec, const Shape& sh, uint32_t sample, bool exact, Sink& s, uint32_t& outside)
{
    const uint8_t* q = rec + 8 + sh.l_shared;
    const uint32_t li = sh.l_indiv;
    uint32_t at = 0;
    s.put('\t');
    for (uint32_t k = 0; k < sh.n_fmt; ++k) {
        uint32_t key = 0, type = 0, count = 0;
        if (read_key(q, li, at, key) || read_vector(q, li, at, type, count, sh.n_sample)) return;     // (not a record shared_text accepted)
        const uint32_t size = count * width_of(type), mine = at + sample * size;
        if (k) s.put(':');
        if (key == d.gt_key && is_int(type)) put_gt(s, q, li, mine, type, count);
        else if (type == kBtChar) {
            uint32_t e = mine;
            while (e < mine + count && load8(q, li, e)) ++e;
            if (e == mine) s.put('.');
            else put_bytes(s, q, mine, e);
        } else if (type == 0) s.put('.');
        else put_numbers(s, q, li, mine, type, count, exact, outside);
        at += sh.n_sample * size;
    }
}

}  // namespace bcftext
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <cmath>
#include <cstdio>

namespace svt {
namespace bcftext {

#if !defined(__HIP_DEVICE_COMPILE__)
// snprintf("%g") of the float widened to double; a nan prints "nan" whatever its sign
inline void float_printf(Sink& s, uint32_t bits)
{
    float f;
    std::memcpy(&f, &bits, 4);
    char buf[48];
    const int n = std::isnan(f) ? std::snprintf(buf, sizeof buf, "nan") : std::snprintf(buf, sizeof buf, "%g", (double)f);
    for (int i = 0; i < n; ++i) s.put((uint8_t)buf[i]);
}
#endif

SVT_HD void put_float(Sink& s, uint32_t bits, bool exact, uint32_t& outside)
{
    if (exact && float_exact_text(bits, s)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    outside = 1;
#else
    if (exact) outside = 1;
    float_printf(s, bits);
#endif
}

// the header's dictionaries by index, made once per stream: the storage behind a TextDict, and the VCF header
struct TextTables {
    std::vector<uint8_t> names, types, cnames, chave;
    std::vector<uint32_t> name_off{0}, cname_off{0};
    uint32_t n_sample = 0, gt_key = kNoKey;
    std::string header;             // the header text without its ,IDX=n attributes and its NUL

    TextDict view() const
    {
        return TextDict{names.data(), name_off.data(), types.data(), cnames.data(), cname_off.data(), chave.data(),
                        (uint32_t)name_off.size() - 1, (uint32_t)cname_off.size() - 1, n_sample, gt_key};
    }
};

// text[0, len) without every ,IDX=<digits> that stands outside quotes in a ## line
inline std::string strip_idx(const uint8_t* text, uint64_t len)
{
    std::string out;
    out.reserve(len);
    bool quoted = false, meta = false;
    for (uint64_t i = 0; i < len; ++i) {
        if (i == 0 || text[i - 1] == '\n') {
            quoted = false;
            meta = i + 1 < len && text[i] == '#' && text[i + 1] == '#';
        }
        if (text[i] == '"') quoted = !quoted;
        if (meta && !quoted && text[i] == ',' && len - i > 5 && std::memcmp(text + i, ",IDX=", 5) == 0 && bcf::is_digit(text[i + 5])) {
            i += 5;
            while (i + 1 < len && bcf::is_digit(text[i + 1])) ++i;
            continue;
        }
        out.push_back((char)text[i]);
    }
    return out;
}

// The dictionaries of the BCF header text[0, len) (no NUL).  A ##FILTER, ##INFO, ##FORMAT or ##contig line with IDX= sits at
// that index; one without sits where svt_bcf.h's writer counts it: PASS is 0, then every new ID in order of appearance, an ID
// of two categories once; contigs in order.  null, or what is wrong with the header
inline const char* make_text_tables(const uint8_t* text, uint64_t len, TextTables& t)
{
    t = TextTables();
    std::vector<std::string> keys{"PASS"}, contigs;
    std::vector<uint8_t> have{1}, types{1, 0, 0};
    std::unordered_map<std::string, uint32_t> key_at{{"PASS", 0}}, contig_at;
    bool chrom_line = false;
    std::string id, type, idx;
    for (uint64_t at = 0; at < len; ) {
        const void* nl = std::memchr(text + at, '\n', len - at);
        const uint64_t end = nl ? (uint64_t)((const uint8_t*)nl - text) + 1 : len;
        const uint8_t* p = text + at;
        const uint64_t n = end - at;
        at = end;
        if (!n || p[0] != '#') return "a line of the header does not begin with '#'";
        if (chrom_line) return "a '#' line behind the #CHROM line";
        static const char* const kKinds[4] = {"##FILTER=<", "##INFO=<", "##FORMAT=<", "##contig=<"};
        for (uint32_t c = 0; c < 4; ++c) {
            const uint64_t lead = std::strlen(kKinds[c]);
            if (n < lead || std::memcmp(p, kKinds[c], lead) != 0 || !bcf::header_field(p, lead, n, "ID", id)) continue;
            int64_t want = -1;
            if (bcf::header_field(p, lead, n, "IDX", idx)) {
                if (idx.empty() || idx.size() > 7 || idx.find_first_not_of("0123456789") != std::string::npos) return "an IDX that is no index";
                want = std::strtol(idx.c_str(), nullptr, 10);
            }
            std::vector<std::string>& names = c == 3 ? contigs : keys;
            std::unordered_map<std::string, uint32_t>& where = c == 3 ? contig_at : key_at;
            std::vector<uint8_t>& held = c == 3 ? t.chave : have;
            uint32_t k;
            auto it = where.find(id);
            if (it != where.end()) {
                k = it->second;
                if (want >= 0 && (uint32_t)want != k) return "an ID with two IDX";      // (PASS is 0, with a line or without)
            } else {
                k = want >= 0 ? (uint32_t)want : (uint32_t)names.size();
                where.emplace(id, k);
            }
            if (k >= names.size()) {
                names.resize(k + 1);
                held.resize(k + 1, 0);
                if (c != 3) types.resize(3 * (k + 1), 0);
            }
            if (held[k] && names[k] != id) return "two IDs at one IDX";
            names[k] = id;
            held[k] = 1;
            if (c == 3) continue;
            uint8_t code = 1;
            if (c) {
                if (!bcf::header_field(p, lead, n, "Type", type)) return "an ##INFO or ##FORMAT line without a Type";
                code = type == "Integer" ? bcf::kTypeInt : type == "Float" ? bcf::kTypeFloat : type == "Flag" ? bcf::kTypeFlag
                       : type == "String" || type == "Character" ? bcf::kTypeString : bcf::kTypeNone;
                if (code == bcf::kTypeNone) return "an ##INFO or ##FORMAT line with a Type that is none";
            }
            if (types[3 * k + c] == bcf::kTypeNone) types[3 * k + c] = code;
        }
        if (n >= 6 && std::memcmp(p, "#CHROM", 6) == 0) {
            chrom_line = true;
            uint32_t tabs = 0;
            for (uint64_t i = 0; i < n; ++i) tabs += p[i] == '\t';
            t.n_sample = tabs > 8 ? tabs - 8 : 0;
        }
    }
    if (!chrom_line) return "the header has no #CHROM line";
    for (uint32_t k = 0; k < keys.size(); ++k) {
        if (!have[k]) types[3 * k] = types[3 * k + 1] = types[3 * k + 2] = 0;
        else if (keys[k] == "GT" && types[3 * k + 2]) t.gt_key = k;
        t.names.insert(t.names.end(), keys[k].begin(), keys[k].end());
        t.name_off.push_back((uint32_t)t.names.size());
    }
    for (const std::string& c : contigs) {
        t.cnames.insert(t.cnames.end(), c.begin(), c.end());
        t.cname_off.push_back((uint32_t)t.cnames.size());
    }
    t.types = types;
    t.names.push_back(0);           // (never empty: data() of an empty vector may be null)
    t.cnames.push_back(0);
    t.chave.push_back(0);
    t.header = strip_idx(text, len);
    if (t.header.empty() || t.header.back() != '\n') t.header.push_back('\n');
    return nullptr;
}

// The stream's frame: magic, l_text, the header text (the NULs at its end dropped) -> the tables; body: where the records begin
inline const char* read_stream_header(const uint8_t* stream, uint64_t len, TextTables& t, uint64_t& body)
{
    if (len < 9 || std::memcmp(stream, "BCF\2\2", 5) != 0) return "no BCF2.2 magic";
    const uint64_t l_text = load32(stream, 9, 5);
    if (l_text > len - 9) return "the header text runs out of the stream";
    uint64_t n = l_text;
    while (n && stream[9 + n - 1] == 0) --n;
    if (std::memchr(stream + 9, 0, n)) return "a NUL inside the header text";
    body = 9 + l_text;
    return make_text_tables(stream + 9, n, t);
}

// offsets[0 .. n]: where the records of stream[body, len) begin, two uint32 read per record.  true where bytes are left that
// hold no whole record (record n + 1 runs out of the stream)
inline bool walk_chain(const uint8_t* stream, uint64_t len, uint64_t body, std::vector<uint64_t>& offsets)
{
    offsets.assign(1, body);
    for (uint64_t at = body; at < len; ) {
        if (len - at < 8) return true;
        const uint64_t size = 8ull + load32(stream + at, 8, 0) + load32(stream + at, 8, 4);
        if (size > len - at) return true;
        at += size;
        offsets.push_back(at);
    }
    return false;
}

// the records [from, to) of one chunk: as many as block_bytes of stream hold, one at the least
inline uint64_t chunk_end(const std::vector<uint64_t>& offsets, uint64_t from, uint64_t block_bytes)
{
    uint64_t to = from + 1;
    while (to + 1 < offsets.size() && offsets[to + 1] - offsets[from] <= block_bytes) ++to;
    return to;
}

// one record's whole line on one thread: shared_text, every sample's column, the newline.  Returns sh.kind
inline uint32_t line_text(const TextDict& d, const uint8_t* rec, uint64_t len, bool exact, Sink& s, Shape& sh)
{
    if (shared_text(d, rec, len, exact, s, sh)) return sh.kind;
    for (uint32_t k = 0; sh.n_fmt && k < sh.n_sample; ++k) sample_text(d, rec, sh, k, exact, s, sh.outside);
    s.put('\n');
    return 0;
}

// what a decoding call leaves for svt_bcf_text_take
struct TextHeld {
    std::vector<uint8_t> text, marks;
    std::vector<uint64_t> offsets;
    void clear()
    {
        std::vector<uint8_t>().swap(text);
        std::vector<uint8_t>().swap(marks);
        std::vector<uint64_t>().swap(offsets);
    }
};

// svt_bcf_text_host without its argument checks: the VCF text (header and lines) into held.text.  `exact`: floats by the
// device's rule first; info.host_lines counts the records it left to snprintf
inline const char* text_host(const uint8_t* stream, uint64_t len, bool exact, uint64_t block_bytes, svt_bcf_text_info& info, TextHeld& held)
{
    TextTables t;
    uint64_t body = 0;
    if (const char* why = read_stream_header(stream, len, t, body)) return why;
    const TextDict d = t.view();
    std::vector<uint64_t> chain;
    const bool cut_short = walk_chain(stream, len, body, chain);
    const uint64_t n = chain.size() - 1;
    info.n_sample = t.n_sample;
    info.header_len = t.header.size();
    held.text.assign(t.header.begin(), t.header.end());
    held.offsets.assign(1, held.text.size());
    held.marks.assign(n, 0);
    for (uint64_t from = 0; from < n; ++info.chunks) {
        const uint64_t to = chunk_end(chain, from, block_bytes);
        for (uint64_t j = from; j < to; ++j) {
            Sink count{nullptr, 0, 0};
            Shape sh;
            if (line_text(d, stream + chain[j], chain[j + 1] - chain[j], exact, count, sh)) {
                info.bad_record = j + 1;
                info.bad_kind = sh.kind;
                return nullptr;
            }
            held.marks[j] = (uint8_t)sh.outside;
            info.host_lines += sh.outside;
            held.offsets.push_back(held.offsets.back() + count.n);
        }
        held.text.resize(held.offsets.back());
        for (uint64_t j = from; j < to; ++j) {
            Sink store{held.text.data() + held.offsets[j], held.offsets[j + 1] - held.offsets[j], 0};
            Shape sh;
            line_text(d, stream + chain[j], chain[j + 1] - chain[j], exact, store, sh);
            if (store.n != store.cap) return "svt_bcf_text: a record's two walks disagree";
        }
        from = to;
    }
    if (cut_short) {
        info.bad_record = n + 1;
        info.bad_kind = SVT_BCF_TEXT_KIND_TRUNCATED;
        return nullptr;
    }
    info.n_records = n;
    return nullptr;
}

}  // namespace bcftext
}  // namespace svt
#endif  // SVT_BCF_TEXT_H

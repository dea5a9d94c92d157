// svt_vcf_cohort_line.h -- a body line of a cohort VCF: what the programs that read such lines share.  The users are
// svt_vcf_paste.h (the character classes and the text-side number helpers), svt_vcf_classify.h and svt_vcf_update_info.h (all of
// it) and svt_vcf_group.h (the line's tabs, POS, QUAL and FORMAT, the field walk, the script's Variant and its writer; its join
// over the whole file has drivers of its own); none of them includes another's header.
//
// Host and device (SVT_HD): the right-strip, the first nine tabs, the checks of POS, QUAL and FORMAT that both rules make on the
// head, the walk over the ':' fields of a column.  Every load is checked against the line's length.  What differs between the
// rules stays in their headers: which columns a line needs, what else the head is read for, their marks.
//
// Host only: the script's Variant in plain C++ (parse_variant, var_string, generic_tail), Python's float(), int() and '%0.2f',
// and the drivers that are the same for every rule, written once over the rule's Block: rule_host, write_block and report.  A
// rule's namespace holds its Block (derived from cohort::Block, with its name and its refusals' texts, which take_block_arguments
// and the entries return) and the functions the drivers find by their arguments: check_head, fast_line, settle_block and write_line.
#ifndef SVT_VCF_COHORT_LINE_H
#define SVT_VCF_COHORT_LINE_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bcf.h"

namespace svt {
namespace cohort {

constexpr uint32_t kMaxLine = 0x7FFFFFFFu, kNone = 0xFFFFFFFFu, kBlock = 256;

SVT_HD bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }         // what str.rstrip() strips
SVT_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

SVT_HD uint32_t stripped_length(const uint8_t* p, uint64_t len)
{
    uint32_t n = len > kMaxLine ? kMaxLine : (uint32_t)len;
    while (n && is_space(p[n - 1])) --n;
    return n;
}

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

// where the first nine tabs of a right-stripped line of n bytes stand: tab[0 .. count), n behind them
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

// column c (1 .. 8) is p[column_begin(t, c, n), t.tab[c]): empty at the line's end where the line has no such column
SVT_HD uint32_t column_begin(const Tabs& t, uint32_t c, uint32_t n) { return t.count >= c ? t.tab[c - 1] + 1 : n; }

// the fields of p[b, e) between the separator `sep`, in order: field(index, begin, end) for each, an empty one included.
// Returns their number
template <class Field>
SVT_HD uint32_t walk_fields(const uint8_t* p, uint32_t b, uint32_t e, uint8_t sep, Field field)
{
    uint32_t idx = 0;
    for (uint32_t at = b; at <= e; ++idx) {
        uint32_t fe = at;
        while (fe < e && p[fe] != sep) ++fe;
        field(idx, at, fe);
        at = fe + 1;
    }
    return idx;
}

// what the first nine columns give both rules; a rule's Head adds what it alone reads
constexpr uint32_t kMaxKeys = 3;
struct Head {
    uint32_t n;                                     // the line's length without its trailing blanks
    uint32_t samples_b;                             // behind the ninth tab (n: no tenth column)
    uint32_t n_fmt;                                 // FORMAT's fields
    uint32_t key_at[kMaxKeys];                      // where the rule's keys stand among them (kNone: nowhere)
    uint32_t slow;
};

SVT_HD void begin_head(uint32_t n, const Tabs& t, Head& h)
{
    h.n = n;
    h.samples_b = t.count == 9 ? t.tab[8] + 1 : n;
    h.n_fmt = h.slow = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMaxKeys; ++k) h.key_at[k] = kNone;
}

// The checks on the head of a line of at least eight columns: POS of 1 to 18 digits and QUAL "." or inside bcf::double_exact
// (else `mark_head`), FORMAT with GT first and the header's keys in the header's order (else `mark_format`).  `keys`: n_keys
// FORMAT keys of two letters side by side, whose places go to h.key_at
// the first half on its own, for a rule that also takes lines of eight columns (svt_vcf_group.h): POS and QUAL of a line of at
// least six tabs
SVT_HD bool pos_qual_exact(const uint8_t* p, const Tabs& t)
{
    const uint32_t pos_b = t.tab[0] + 1, pos_e = t.tab[1], qual_b = t.tab[4] + 1, qual_e = t.tab[5];
    bool digits = pos_e > pos_b && pos_e - pos_b <= 18;
    for (uint32_t i = pos_b; i < pos_e; ++i) digits = digits && is_digit(p[i]);
    double qual;
    return digits && (bcf::is_dot(p, qual_b, qual_e) || !bcf::double_exact(p, qual_b, qual_e, qual));
}

SVT_HD void check_head(const uint8_t* p, const Tabs& t, const uint8_t* table, uint32_t table_len, uint32_t mark_head, uint32_t mark_format,
                       const char* keys, uint32_t n_keys, Head& h)
{
    if (!pos_qual_exact(p, t)) h.slow |= mark_head;
    uint32_t last = kNone;
    h.n_fmt = walk_fields(p, column_begin(t, 8, h.n), t.tab[8], ':', [&](uint32_t idx, uint32_t b, uint32_t e) {
        const uint32_t k = table_index(table, table_len, p, b, e);
        if (k == kNone || (last == kNone ? k != 0 : k <= last)) h.slow |= mark_format;
        last = k;
#pragma unroll
        for (uint32_t w = 0; w < kMaxKeys; ++w)
            if (w < n_keys && bytes_are(p, b, e, keys + 2 * w, 2)) h.key_at[w] = idx;
    });
}

}  // namespace cohort
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "svt_vcf_lines.h"

namespace svt {
namespace cohort {

// ---- Python's float(), int() and '%0.2f' of the scripts
inline void strip(const uint8_t* p, uint32_t& b, uint32_t& e)
{
    while (b < e && is_space(p[b])) ++b;
    while (e > b && is_space(p[e - 1])) --e;
}

inline bool word_is(const uint8_t* p, uint32_t b, uint32_t e, const char* w)
{
    if (e - b != std::strlen(w)) return false;
    for (uint32_t i = 0; i < e - b; ++i)
        if ((p[b + i] | 0x20) != (uint8_t)w[i]) return false;
    return true;
}

// float(token) of Python 2: blanks around it, a sign, inf / infinity / nan, or decimal digits with a point and an exponent
inline bool py_float(const uint8_t* p, uint32_t b, uint32_t e, double& v)
{
    strip(p, b, e);
    uint32_t i = b;
    if (i < e && (p[i] == '+' || p[i] == '-')) ++i;
    if (word_is(p, i, e, "inf") || word_is(p, i, e, "infinity") || word_is(p, i, e, "nan")) {
        v = word_is(p, i, e, "nan") ? std::nan("") : HUGE_VAL;
        if (p[b] == '-') v = -v;
        return true;
    }
    uint32_t digits = 0;
    while (i < e && is_digit(p[i])) { ++i; ++digits; }
    if (i < e && p[i] == '.') {
        ++i;
        while (i < e && is_digit(p[i])) { ++i; ++digits; }
    }
    if (!digits) return false;
    if (i < e && (p[i] | 0x20) == 'e') {
        ++i;
        if (i < e && (p[i] == '+' || p[i] == '-')) ++i;
        if (i == e || !is_digit(p[i])) return false;
        while (i < e && is_digit(p[i])) ++i;
    }
    if (i != e) return false;
    const std::string token((const char*)p + b, e - b);
    v = std::strtod(token.c_str(), nullptr);
    return true;
}

// str(int(token)): blanks around it, a sign, decimal digits of any number
inline bool py_int_text(const uint8_t* p, uint32_t b, uint32_t e, std::string& out)
{
    strip(p, b, e);
    const bool neg = b < e && p[b] == '-';
    if (b < e && (p[b] == '+' || p[b] == '-')) ++b;
    if (b == e) return false;
    for (uint32_t i = b; i < e; ++i)
        if (!is_digit(p[i])) return false;
    while (e - b > 1 && p[b] == '0') ++b;
    out.clear();
    if (neg && p[b] != '0') out += '-';
    out.append((const char*)p + b, e - b);
    return true;
}

inline std::string fixed2(double v)
{
    if (std::isnan(v)) return "nan";
    char buf[400];
    std::snprintf(buf, sizeof buf, "%0.2f", v);
    return buf;
}

// "V<id>\n" / "F<id>\n" per INFO id (F: a Flag)
inline bool parse_info_table(const uint8_t* p, uint64_t n, std::vector<std::pair<std::string, bool>>& info)
{
    info.clear();
    for (uint64_t at = 0; at < n;) {
        const void* nl = std::memchr(p + at, '\n', n - at);
        if (!nl || (p[at] != 'V' && p[at] != 'F')) return false;
        const uint64_t e = (uint64_t)((const uint8_t*)nl - p);
        info.emplace_back(std::string((const char*)p + at + 1, e - at - 1), p[at] == 'F');
        at = e + 1;
    }
    return true;
}

// "<id>\n" per FORMAT id, GT first
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

// ---- one block and the script's Variant of one of its lines
// why a line ends the run: the kind is the rule's (SVT_CLASSIFY_BAD_*, SVT_UPDATE_INFO_BAD_*)
struct Bad {
    uint32_t kind = 0, sample = kNone;
    std::string text;
};

// the kinds parse_variant sets, which every rule's report names alike
constexpr uint32_t kBadColumns = 1, kBadPos = 2, kBadQual = 3, kBadFormat = 4, kBadEight = 9;
static_assert(SVT_CLASSIFY_BAD_COLUMNS == kBadColumns && SVT_CLASSIFY_BAD_POS == kBadPos && SVT_CLASSIFY_BAD_QUAL == kBadQual &&
                  SVT_CLASSIFY_BAD_FORMAT == kBadFormat && SVT_UPDATE_INFO_BAD_COLUMNS == kBadColumns && SVT_UPDATE_INFO_BAD_POS == kBadPos &&
                  SVT_UPDATE_INFO_BAD_QUAL == kBadQual && SVT_UPDATE_INFO_BAD_FORMAT == kBadFormat && SVT_UPDATE_INFO_BAD_EIGHT == kBadEight &&
                  SVT_GROUP_BAD_COLUMNS == kBadColumns && SVT_GROUP_BAD_POS == kBadPos && SVT_GROUP_BAD_QUAL == kBadQual &&
                  SVT_GROUP_BAD_FORMAT == kBadFormat && SVT_GROUP_BAD_EIGHT == kBadEight,
              "svt_classify_info, svt_update_info_report and svt_group_report name a line's first columns alike");

// the text under its line table, the header's FORMAT ids and (the writer) its INFO ids; a rule's Block adds its tables
struct Block {
    const uint8_t* text = nullptr;
    uint64_t len = 0;
    const svt_tbx_line* lines = nullptr;
    uint64_t n_table = 0;
    const uint8_t* format_table = nullptr;
    std::vector<std::string> formats;
    std::vector<std::pair<std::string, bool>> info; // the header's INFO ids in its order, and whether the Type is Flag
    bool skipped(uint64_t) const { return false; }  // line j is not the rule's
};

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

// What every rule's take_arguments does with the text and the FORMAT table: `info` cleared and `b` filled, or what is wrong with
// them in the rule's words (B::kLengthWhy, B::kFormatWhy).  `others`: the pointers that are the rule's alone are there
template <class B, class Info>
const char* take_block_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len, bool others,
                                 Info* info, B& b)
{
    if (!info || !others || (len && !text) || !format_table) return "null argument";
    *info = Info();
    if (len > kMaxLine) return B::kLengthWhy;
    if (format_len > 0xFFFFu || !parse_format_table(format_table, format_len, b.formats)) return B::kFormatWhy;
    b.text = text;
    b.len = len;
    b.format_table = format_table;
    b.pr.n_samples = n_samples;
    b.pr.format_len = (uint32_t)format_len;
    return nullptr;
}

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
    walk_fields(p, b, e, c, [&](uint32_t, uint32_t fb, uint32_t fe) { out.emplace_back(fb, fe); });
}

// Variant(v, vcf) of the script, in its order; `samples`: the n_samples sample columns too (the writer of an unmarked line copies
// them).  `script_order`: a line of fewer than eight columns ends as in a script that reads POS and QUAL before it counts the
// columns (update_info.py), and one of seven columns gets the script's own message
inline bool parse_variant(const Block& b, uint32_t n_samples, const uint8_t* p, uint64_t len, bool samples, bool script_order, Variant& v, Bad& bad)
{
    const uint32_t n = stripped_length(p, len);
    split(p, 0, n, '\t', v.col);
    auto column = [&](size_t k) { return bytes(p, v.col[k].first, v.col[k].second); };
    auto pos_is_bad = [&]() {
        if (py_int_text(p, v.col[1].first, v.col[1].second, v.pos)) return false;
        bad.kind = kBadPos;
        bad.text = column(1);
        return true;
    };
    double q = 0.0;
    auto qual_is_bad = [&]() {
        if (bcf::is_dot(p, v.col[5].first, v.col[5].second) || py_float(p, v.col[5].first, v.col[5].second, q)) return false;
        bad.kind = kBadQual;
        bad.text = column(5);
        return true;
    };
    if (len > kMaxLine || v.col.size() < 8) {
        bad.kind = kBadColumns;
        if (!script_order || len > kMaxLine || v.col.size() < 2 || pos_is_bad() || v.col.size() < 6 || qual_is_bad()) return false;
        if (v.col.size() == 7) bad.kind = kBadEight;
        return false;
    }
    v.chrom = column(0);
    if (pos_is_bad()) return false;
    v.id = column(2);
    v.ref = column(3);
    v.alt = column(4);
    if (qual_is_bad()) return false;
    v.qual = fixed2(q);
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
        v.value.assign(n_samples, std::vector<std::string>(b.formats.size()));
        v.has.assign(n_samples, std::vector<uint8_t>(b.formats.size(), 0));
        for (uint32_t s = 0; s < n_samples; ++s) {
            v.active[0] = v.has[s][0] = 1;
            if (9 + (size_t)s >= v.col.size()) {
                v.value[s][0] = "./.";
                continue;
            }
            split(p, v.col[9 + s].first, v.col[9 + s].second, ':', fields);
            v.value[s][0] = bytes(p, fields[0].first, fields[0].second);
            for (size_t j = 0; j < keys.size() && j < fields.size(); ++j) {
                if (key_index[j] == kNone) {
                    bad.kind = kBadFormat;
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

// FORMAT and the sample columns of a line parsed with its samples: the active keys in the header's order, "." where a sample
// lacks one
inline std::string generic_tail(const Block& b, const Variant& v)
{
    std::string out;
    auto row = [&](auto field) {
        bool first = true;
        for (size_t k = 0; k < b.formats.size(); ++k) {
            if (!v.active[k]) continue;
            if (!first) out += ':';
            first = false;
            out += field(k);
        }
    };
    row([&](size_t k) { return b.formats[k]; });
    out += '\t';
    for (size_t s = 0; s < v.value.size(); ++s) {
        if (s) out += '\t';
        row([&](size_t k) { return v.has[s][k] ? v.value[s][k] : std::string("."); });
    }
    return out;
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

// the head of the line p[0, len) by the rule's check_head
template <class H, class B>
H head_of(const B& b, const uint8_t* p, uint64_t len)
{
    const uint32_t n = stripped_length(p, len);
    Tabs t;
    find_tabs(p, n, t);
    H h;
    check_head(p, n, len > kMaxLine, t, b.format_table, b.pr.format_len, h);
    return h;
}

// ---- the drivers, once for every rule.  B is the rule's Block; fast_line, settle_block and write_line are the rule's
template <class Info>
void report(Info& info, uint64_t bad_line, const Bad& bad)
{
    info.bad_line = bad_line;
    info.bad_kind = bad.kind;
    info.bad_sample = bad.sample;
    std::memset(info.bad_text, 0, sizeof info.bad_text);
    std::memcpy(info.bad_text, bad.text.data(), std::min(bad.text.size(), sizeof info.bad_text - 1));
}

// what follows the rule on both engines: the marked lines settled in plain C++, and the first line the script dies on reported
template <class B, class Line, class Info>
void settle(const B& b, Line* results, Info& info)
{
    Bad bad;
    if (const uint64_t bad_line = settle_block(b, results, info, bad)) report(info, bad_line, bad);
}

// one block on the host: the line table, the host twin of the kernel line by line, the marked lines settled
template <class B, class Line, class Info>
const char* rule_host(B& b, std::vector<svt_tbx_line>& table, Line* results, uint64_t capacity, uint64_t* n_lines, Info& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    b.lines = table.data();
    b.n_table = table.size();
    *n_lines = table.size();
    if (table.size() > capacity) return B::kCapacityWhy;
    for (uint64_t j = 0; j < b.n_table; ++j)
        if (!b.skipped(j)) results[j] = fast_line(b, b.text + table[j].off, table[j].len);
    settle(b, results, info);
    return nullptr;
}

// the writer's entry: the block's output into `out`, out_off[0 .. n_lines]
template <class B, class Line, class Info>
const char* write_block(B& b, std::vector<svt_tbx_line>& table, const Line* results, uint64_t n_lines, uint64_t* out_off, std::string& out, Info& info)
{
    table.resize(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    if (table.size() != n_lines) return B::kWriteWhy;
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

}  // namespace cohort
}  // namespace svt
#endif  // SVT_VCF_COHORT_LINE_H

// svt_vcf_group.h -- BND mates grouped in front of the paste: the per-line rule, its host twin, the join as the script runs it,
// the plain C++ of the lines outside the rule's envelope and the writer of the output text (DESIGN 3.4,
// include/svtyper_reads.h: svt_group_line, svt_group_out).
//
// ONE piece of source for both places that run the rule: scan_line is compiled for the host (any C++17 compiler: this is where
// it is proven against goldens made from the reference's scripts/vcf_group_multiline.py, and sanitised) and for the device
// (svt_vcf_group_kernel.h, one lane per line).  Every load is checked against the line's length.  What a cohort line is to every
// rule (its tabs, POS, QUAL and FORMAT, the script's Variant) is svt_vcf_cohort_line.h's; the hash of an ID is
// svt_bam_first_rules.h's FNV-1a.
//
// What the script does: every body line becomes a Variant; INFO's SVTYPE is read.  A line that is no BND is written in place
// after int(END), map(int, CIPOS.split(',')) and the same of CIEND.  A BND whose MATEID is a key of the breakend dictionary is
// the second of a pair: CIPOS of both lines is read, the stored line is written and then this one with the stored line's QUAL,
// FORMAT and sample columns; any other BND is stored under its own ID and nothing is written.  Entries are never removed.
//
// The envelope of the rule (scan_line decides a line inside it; anything else marks the line, SVT_GROUP_SLOW_*, and decide
// settles it in plain C++ over cohort::parse_variant ON BOTH ENGINES, nothing is guessed):
//   HEAD    at least eight columns, POS of 1 to 18 digits, QUAL "." or inside bcf::double_exact
//   FORMAT  where there is a ninth column: GT first and the header's keys in the header's order
//   BARE    every key the script reads of the line (SVTYPE; MATEID and CIPOS of a BND; END, CIPOS and CIEND of any other line)
//           is absent or has a '='.  Dictionary semantics are inside: the last item of a key counts, and its value ends at a
//           second '='
//   TOKEN   END, and every comma-separated token of a CIPOS or CIEND that is read, is an optional '-' and one to nine digits
//           (int() also takes a '+', blanks around the token and more digits: those are decide's)
//   ALT     the ALT of a BND is not empty (the script indexes its last character when the line pairs)
// Inside the envelope a line can end the run only for a key that is not there (KeyError): svt_group_line.bad names it, and a BND
// without CIPOS is left without SVT_GROUP_CI, which ends the run only if the line pairs.
#ifndef SVT_VCF_GROUP_H
#define SVT_VCF_GROUP_H

#include <stdint.h>

#include "../../include/svtyper_reads.h"
#include "svt_bam_first_rules.h"
#include "svt_vcf_cohort_line.h"

namespace svt {
namespace group {

using cohort::bytes_are;
using cohort::is_digit;
using cohort::kMaxLine;
using cohort::kNone;
using cohort::Tabs;

constexpr uint32_t kKeys = 5, kMaxDigits = 9;
constexpr uint32_t kAbsent = 0, kValue = 1, kBare = 2;

struct Params {
    uint32_t n_samples, format_len;
};

// the five keys the script reads, as INFO's dictionary holds them: the last item of each (indexed by unrolled constants only)
struct Keys {
    uint32_t b[kKeys], e[kKeys], state[kKeys];
};

SVT_HD uint32_t key_index(const uint8_t* p, uint32_t b, uint32_t e)
{
    if (bytes_are(p, b, e, "SVTYPE", 6)) return SVT_GROUP_KEY_SVTYPE;
    if (bytes_are(p, b, e, "MATEID", 6)) return SVT_GROUP_KEY_MATEID;
    if (bytes_are(p, b, e, "END", 3)) return SVT_GROUP_KEY_END;
    if (bytes_are(p, b, e, "CIPOS", 5)) return SVT_GROUP_KEY_CIPOS;
    if (bytes_are(p, b, e, "CIEND", 5)) return SVT_GROUP_KEY_CIEND;
    return kNone;
}

// INFO p[b, e): a.split('=') of every item; [0] is the key, [1] the value, True where there is none
SVT_HD void read_keys(const uint8_t* p, uint32_t b, uint32_t e, Keys& k)
{
#pragma unroll
    for (uint32_t w = 0; w < kKeys; ++w) k.b[w] = k.e[w] = e, k.state[w] = kAbsent;
    cohort::walk_fields(p, b, e, ';', [&](uint32_t, uint32_t at, uint32_t fe) {
        uint32_t eq = at;
        while (eq < fe && p[eq] != '=') ++eq;
        const uint32_t which = key_index(p, at, eq);
        if (which == kNone) return;
        const bool bare = eq == fe;
        const uint32_t vb = bare ? fe : eq + 1;
        uint32_t ve = vb;
        while (ve < fe && p[ve] != '=') ++ve;
#pragma unroll
        for (uint32_t w = 0; w < kKeys; ++w)
            if (which == w) k.b[w] = vb, k.e[w] = ve, k.state[w] = bare ? kBare : kValue;
    });
}

// an optional '-' and one to kMaxDigits digits
SVT_HD bool strict_int(const uint8_t* p, uint32_t b, uint32_t e)
{
    if (b < e && p[b] == '-') ++b;
    if (e == b || e - b > kMaxDigits) return false;
    for (uint32_t i = b; i < e; ++i)
        if (!is_digit(p[i])) return false;
    return true;
}

SVT_HD bool strict_list(const uint8_t* p, uint32_t b, uint32_t e)
{
    bool all = true;
    cohort::walk_fields(p, b, e, ',', [&](uint32_t, uint32_t at, uint32_t fe) { all = all && strict_int(p, at, fe); });
    return all;
}

// what the script reads of a key of a line that is no BND, in its order: absent is the line's end unless an earlier key was
SVT_HD void read_own(const uint8_t* p, uint32_t state, uint32_t b, uint32_t e, bool list, uint32_t key, uint32_t& slow, uint32_t& bad)
{
    if (state == kBare) slow |= SVT_GROUP_SLOW_BARE;
    else if (state == kAbsent) {
        if (!bad) bad = SVT_GROUP_BAD_KEY | key << 8;
    } else if (!(list ? strict_list(p, b, e) : strict_int(p, b, e))) slow |= SVT_GROUP_SLOW_TOKEN;
}

// The rule: the record of the line p[0, len) that begins at `off` of the text.  A marked line's record holds its place, its
// stripped length and its marks alone
SVT_HD svt_group_line scan_line(const uint8_t* p, uint64_t off, uint64_t len, const uint8_t* table, uint32_t table_len)
{
    svt_group_line r = svt_group_line();
    const uint32_t n = cohort::stripped_length(p, len);
    r.off = off;
    r.len = n;
    Tabs t;
    cohort::find_tabs(p, n, t);
    if (len > kMaxLine || t.count < 7) {
        r.slow = SVT_GROUP_SLOW_HEAD;
        return r;
    }
    uint32_t slow = 0, flags = 0, bad = 0, mate_b = 0, mate_n = 0;
    if (!cohort::pos_qual_exact(p, t)) slow |= SVT_GROUP_SLOW_HEAD;
    if (t.count >= 8) {
        uint32_t last = kNone;
        cohort::walk_fields(p, t.tab[7] + 1, t.tab[8], ':', [&](uint32_t, uint32_t b, uint32_t e) {
            const uint32_t k = cohort::table_index(table, table_len, p, b, e);
            if (k == kNone || (last == kNone ? k != 0 : k <= last)) slow |= SVT_GROUP_SLOW_FORMAT;
            last = k;
        });
    }
    Keys k;
    read_keys(p, t.tab[6] + 1, t.tab[7], k);
    constexpr uint32_t SV = SVT_GROUP_KEY_SVTYPE, MATE = SVT_GROUP_KEY_MATEID, END = SVT_GROUP_KEY_END, CIPOS = SVT_GROUP_KEY_CIPOS,
                       CIEND = SVT_GROUP_KEY_CIEND;
    if (k.state[SV] == kBare) slow |= SVT_GROUP_SLOW_BARE;
    else if (k.state[SV] == kAbsent) bad = SVT_GROUP_BAD_KEY | SV << 8;
    else if (bytes_are(p, k.b[SV], k.e[SV], "BND", 3)) {
        flags |= SVT_GROUP_BND;
        if (t.tab[4] == t.tab[3] + 1) slow |= SVT_GROUP_SLOW_ALT;
        if (k.state[MATE] == kBare) slow |= SVT_GROUP_SLOW_BARE;
        else if (k.state[MATE] == kAbsent) bad = SVT_GROUP_BAD_KEY | MATE << 8;
        else {
            flags |= SVT_GROUP_HAS_MATE;
            mate_b = k.b[MATE];
            mate_n = k.e[MATE] - k.b[MATE];
        }
        if (k.state[CIPOS] == kBare) slow |= SVT_GROUP_SLOW_BARE;
        else if (k.state[CIPOS] == kValue) {
            if (strict_list(p, k.b[CIPOS], k.e[CIPOS])) flags |= SVT_GROUP_CI;
            else slow |= SVT_GROUP_SLOW_TOKEN;
        }
    } else {
        read_own(p, k.state[END], k.b[END], k.e[END], false, END, slow, bad);
        read_own(p, k.state[CIPOS], k.b[CIPOS], k.e[CIPOS], true, CIPOS, slow, bad);
        read_own(p, k.state[CIEND], k.b[CIEND], k.e[CIEND], true, CIEND, slow, bad);
        if (!bad) flags |= SVT_GROUP_CI;
    }
    if (slow) {
        r.slow = slow;
        return r;
    }
    r.id_b = t.tab[1] + 1;
    r.id_n = t.tab[2] - r.id_b;
    r.mate_b = mate_b;
    r.mate_n = mate_n;
    r.flags = flags;
    r.bad = bad;
    return r;
}

// the hash the device sorts the BND lines by, and looks a MATEID up with
SVT_HD uint64_t id_hash(const uint8_t* p, uint32_t b, uint32_t n, uint64_t mask) { return bfr::fnv1a(p + b, n) & mask; }

// a record's ID and MATEID lie inside its line, and the line inside the text
SVT_HD bool spans_inside(const svt_group_line& r, uint64_t text_len)
{
    return r.off <= text_len && r.len <= text_len - r.off && r.id_b <= r.len && r.id_n <= r.len - r.id_b && r.mate_b <= r.len &&
           r.mate_n <= r.len - r.mate_b;
}

SVT_HD bool same_bytes(const uint8_t* a, uint32_t an, const uint8_t* b, uint32_t bn)
{
    if (an != bn) return false;
    for (uint32_t i = 0; i < an; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

}  // namespace group
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "svt_vcf_lines.h"

namespace svt {
namespace group {

using cohort::Bad;
using cohort::Variant;

struct Block : cohort::Block {
    static constexpr const char* kName = "svt_vcf_group";
    static constexpr const char* kCapacityWhy = "svt_vcf_group: capacity is below the number of lines";
    static constexpr const char* kLengthWhy = "svt_vcf_group: the body holds less than 2^31 bytes";
    static constexpr const char* kFormatWhy = "svt_vcf_group: format_table is \"<id>\\n\" per id, GT first";
    Params pr = Params();
};

inline const char* kKeyNames[kKeys] = {"SVTYPE", "MATEID", "END", "CIPOS", "CIEND"};

inline const char* take_arguments(const uint8_t* text, uint64_t len, uint32_t n_samples, const uint8_t* format_table, uint64_t format_len,
                                  const svt_group_line* lines, const uint64_t* n_lines, const svt_group_out* plan, const uint64_t* n_plan,
                                  svt_group_report* report, Block& b)
{
    return cohort::take_block_arguments(text, len, n_samples, format_table, format_len, n_lines && n_plan && lines && plan, report, b);
}

// what the join reads of a line: views into the text
struct Resolved {
    bool bnd = false, has_mate = false, alt_empty = false;
    std::string_view id, mate;
    Bad own, ci;                                    // kind != 0: the script dies on the line; when the line pairs
};

inline Bad bad_key(uint32_t kind, uint32_t key)
{
    Bad bad;
    bad.kind = kind;
    bad.text = kKeyNames[key];
    return bad;
}

// map(int, value.split(',')) of Python 2, or int(value): the first token int() refuses
inline bool py_ints(const uint8_t* p, uint32_t b, uint32_t e, bool list, Bad& bad)
{
    bool all = true;
    std::string text;
    auto token = [&](uint32_t, uint32_t at, uint32_t fe) {
        if (!all || cohort::py_int_text(p, at, fe, text)) return;
        all = false;
        bad.kind = SVT_GROUP_BAD_NUMBER;
        bad.text = cohort::bytes(p, at, fe);
    };
    if (list) cohort::walk_fields(p, b, e, ',', token);
    else token(0, b, e);
    return all;
}

// INFO[key] read as the script reads an interval: KeyError, AttributeError of True.split, ValueError of int()
inline bool py_interval(const uint8_t* p, const Keys& k, uint32_t key, Bad& bad)
{
    if (k.state[key] == kAbsent) bad = bad_key(SVT_GROUP_BAD_KEY, key);
    else if (k.state[key] == kBare) bad = bad_key(SVT_GROUP_BAD_BARE, key);
    else return py_ints(p, k.b[key], k.e[key], true, bad);
    return false;
}

// The whole of one line in plain C++, as the script reads it, in the script's order
inline void decide(const Block& b, const uint8_t* p, uint64_t len, Resolved& r)
{
    r = Resolved();
    Variant v;
    if (!cohort::parse_variant(b, b.pr.n_samples, p, len, true, true, v, r.own)) return;
    r.id = std::string_view((const char*)p + v.col[2].first, v.col[2].second - v.col[2].first);
    r.alt_empty = v.alt.empty();
    Keys k;
    read_keys(p, v.col[7].first, v.col[7].second, k);
    constexpr uint32_t SV = SVT_GROUP_KEY_SVTYPE, MATE = SVT_GROUP_KEY_MATEID, END = SVT_GROUP_KEY_END;
    if (k.state[SV] == kAbsent) {
        r.own = bad_key(SVT_GROUP_BAD_KEY, SV);
        return;
    }
    r.bnd = k.state[SV] == kValue && bytes_are(p, k.b[SV], k.e[SV], "BND", 3);
    if (r.bnd) {
        if (k.state[MATE] == kAbsent) {
            r.own = bad_key(SVT_GROUP_BAD_KEY, MATE);
            return;
        }
        r.has_mate = k.state[MATE] == kValue;      // (True is no key of a dictionary of strings)
        r.mate = std::string_view((const char*)p + k.b[MATE], k.e[MATE] - k.b[MATE]);
        py_interval(p, k, SVT_GROUP_KEY_CIPOS, r.ci);
        return;
    }
    if (k.state[END] == kAbsent) r.own = bad_key(SVT_GROUP_BAD_KEY, END);
    else if (k.state[END] == kValue && !py_ints(p, k.b[END], k.e[END], false, r.own)) return;      // (int(True) is 1)
    else if (py_interval(p, k, SVT_GROUP_KEY_CIPOS, r.own)) py_interval(p, k, SVT_GROUP_KEY_CIEND, r.own);
}

// the same of a line the rule decided, from its record
inline void resolve(const Block& b, const svt_group_line& l, Resolved& r)
{
    const uint8_t* p = b.text + l.off;
    if (l.slow) {
        decide(b, p, l.len, r);
        return;
    }
    r = Resolved();
    r.bnd = (l.flags & SVT_GROUP_BND) != 0;
    r.has_mate = (l.flags & SVT_GROUP_HAS_MATE) != 0;
    r.id = std::string_view((const char*)p + l.id_b, l.id_n);
    r.mate = std::string_view((const char*)p + l.mate_b, l.mate_n);
    if (l.bad) r.own = bad_key(l.bad & 255u, l.bad >> 8);
    if (r.bnd && !(l.flags & SVT_GROUP_CI)) r.ci = bad_key(SVT_GROUP_BAD_KEY, SVT_GROUP_KEY_CIPOS);
}

inline bool records_inside(const Block& b, const svt_group_line* lines, uint64_t n)
{
    for (uint64_t j = 0; j < n; ++j)
        if (!spans_inside(lines[j], b.len)) return false;
    return true;
}

// The join as the script runs it, over the records of either engine: the breakend dictionary keyed by ID bytes, the last store
// wins, nothing is removed.  The plan in output order; the first line the script dies on ends it and is reported.  Nothing is
// kept per line: a stored line is resolved again when a line pairs with it (a marked one by decide once more; host_lines counts
// a line once)
inline void join(const Block& b, const svt_group_line* lines, uint64_t n, svt_group_out* plan, uint64_t* n_plan, svt_group_report& report)
{
    std::unordered_map<std::string_view, uint32_t> stored;
    uint64_t out = 0;
    report.host_join = 1;
    Resolved r, first;
    Bad alt;
    alt.kind = SVT_GROUP_BAD_ALT;
    for (uint64_t j = 0; j < n; ++j) {
        resolve(b, lines[j], r);
        report.host_lines += lines[j].slow != 0;
        report.n_bnd += r.bnd;
        const Bad* bad = r.own.kind ? &r.own : nullptr;
        if (!bad && !r.bnd) plan[out++] = svt_group_out{(uint32_t)j, (uint32_t)j};
        else if (!bad) {
            const auto it = r.has_mate ? stored.find(r.mate) : stored.end();
            if (it == stored.end()) {
                stored[r.id] = (uint32_t)j;
                continue;
            }
            const uint32_t a = it->second;
            resolve(b, lines[a], first);
            bad = first.ci.kind ? &first.ci : r.ci.kind ? &r.ci : first.alt_empty || r.alt_empty ? &alt : nullptr;
            if (!bad) {
                plan[out++] = svt_group_out{a, a};
                plan[out++] = svt_group_out{(uint32_t)j, a};
            }
        }
        if (bad) {
            cohort::report(report, j + 1, *bad);
            break;
        }
    }
    *n_plan = out;
}

// the whole call on the host: the line table, the host twin of the scan kernel line by line, the join
inline const char* group_host(Block& b, svt_group_line* lines, uint64_t capacity, uint64_t* n_lines, svt_group_out* plan, uint64_t* n_plan,
                              svt_group_report& report)
{
    std::vector<svt_tbx_line> table(tbx::count_lines(b.text, b.len));
    tbx::lines_host(b.text, b.len, table.data());
    *n_lines = table.size();
    *n_plan = 0;
    if (table.size() > capacity) return Block::kCapacityWhy;
    if (table.size() >> 31) return "svt_vcf_group: too many lines in one call (< 2^31)";
    for (uint64_t j = 0; j < table.size(); ++j) lines[j] = scan_line(b.text + table[j].off, table[j].off, table[j].len, b.format_table, b.pr.format_len);
    join(b, lines, table.size(), plan, n_plan, report);
    return nullptr;
}

// The writer: entry {line, source} is get_var_string of `line` with the QUAL, the FORMAT and the sample columns of `source`
inline const char* write_plan(const Block& b, const svt_group_line* lines, uint64_t n_lines, const svt_group_out* plan, uint64_t n_plan,
                              uint64_t* out_off, std::string& out, svt_group_report& report)
{
    if (!records_inside(b, lines, n_lines)) return "svt_vcf_group_write: a record's line is not inside the text";
    for (uint64_t j = 0; j < n_plan; ++j)
        if (plan[j].line >= n_lines || plan[j].source >= n_lines) return "svt_vcf_group_write: a plan entry names no line";
    out.clear();
    out_off[0] = 0;
    Bad bad;
    for (uint64_t j = 0; j < n_plan; ++j) {
        const svt_group_line &l = lines[plan[j].line], &s = lines[plan[j].source];
        const bool own = plan[j].line == plan[j].source;
        Variant v, from;
        bool ok = cohort::parse_variant(b, b.pr.n_samples, b.text + l.off, l.len, own, true, v, bad);
        if (ok && !own) {
            ok = cohort::parse_variant(b, b.pr.n_samples, b.text + s.off, s.len, true, true, from, bad);
            v.qual = from.qual;
        }
        if (!ok) {
            cohort::report(report, j + 1, bad);
            for (uint64_t k = j; k < n_plan; ++k) out_off[k + 1] = out_off[j];
            break;
        }
        cohort::var_string(b, v, cohort::generic_tail(b, own ? v : from), out);
        out_off[j + 1] = out.size();
    }
    report.out_len = out.size();
    return nullptr;
}

}  // namespace group
}  // namespace svt
#endif  // SVT_VCF_GROUP_H

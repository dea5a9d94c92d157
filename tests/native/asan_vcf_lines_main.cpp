// asan_vcf_lines_main.cpp -- svtyper_amd/csrc/svt_vcf_lines.h (the per-line rule, the host line table, the order and the gather)
// and svt_tbx_index.h (the index fold) compiled into a stand-alone program with -fsanitize=address,undefined
// (tests/test_vcf_lines_native.py).  Every text lies in a heap buffer of exactly its length: no slack behind it.
//
// Input, one case per line:  T <text hex or -> <expected rows "off,len,beg,end,chrom_len,flags;..." or -> <sorted text hex, - (empty), or ! (not sortable)>
//                            P <text hex>     every prefix of the text through the table, the order, the gather and the fold
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_tbx_index.h"
#include "svt_vcf_lines.h"

namespace tbx = svt::tbx;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

static int failures = 0;
static void failed(const std::string& what)
{
    std::cout << "FAILED " << what << "\n";
    ++failures;
}

struct Run {
    std::unique_ptr<uint8_t[]> text;        // exactly len bytes
    uint64_t len = 0;
    std::vector<svt_tbx_line> lines;
    std::vector<uint8_t> sorted;
    uint64_t bad_line = 0;
};

// the table, the order and the gather of `bytes`, and the fold over both texts; false where the table does not tile the text
static bool run(const std::vector<uint8_t>& bytes, Run& r)
{
    r.len = bytes.size();
    r.text.reset(new uint8_t[r.len]);
    for (uint64_t i = 0; i < r.len; ++i) r.text[i] = bytes[i];
    const uint64_t n = tbx::count_lines(r.text.get(), r.len);
    r.lines.assign(n, svt_tbx_line());
    tbx::lines_host(r.text.get(), r.len, r.lines.data());
    uint64_t at = 0;
    for (const svt_tbx_line& l : r.lines) {
        if (l.off != at || l.len == 0 || l.len > r.len - at) return false;
        at += l.len;
    }
    if (at != r.len) return false;
    std::vector<uint64_t> members((r.len + 99) / 100 + 1);
    for (uint64_t k = 0; k < members.size(); ++k) members[k] = 61 * k;
    std::vector<uint8_t> index;
    uint32_t kind = 0;
    (void)tbx::build(r.text.get(), nullptr, r.lines.data(), n, r.len, members.data(), members.size() - 1, 100, index, kind);
    std::vector<uint64_t> perm(n), dst_off;
    r.bad_line = tbx::sort_order(r.text.get(), r.lines.data(), n, perm.data());
    r.sorted.clear();
    if (r.bad_line) return true;
    if (tbx::gather_plan(r.len, r.lines.data(), n, perm.data(), n, r.len, dst_off)) return false;
    std::unique_ptr<uint8_t[]> out(new uint8_t[r.len]);
    tbx::gather_host(r.text.get(), r.lines.data(), perm.data(), n, dst_off.data(), out.get());
    r.sorted.assign(out.get(), out.get() + r.len);
    std::vector<svt_tbx_line> written(n);
    for (uint64_t j = 0; j < n; ++j) {
        written[j] = r.lines[perm[j]];
        written[j].off = dst_off[j];
    }
    (void)tbx::build(out.get(), nullptr, written.data(), n, r.len, members.data(), members.size() - 1, 100, index, kind);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_prefixes = 0, n_lines = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind, text_hex, want_rows, want_sorted;
        fields >> kind >> text_hex >> want_rows >> want_sorted;
        const std::vector<uint8_t> text = unhex(text_hex);
        Run r;
        if (kind == "T") {
            ++n_cases;
            if (!run(text, r)) { failed("case " + std::to_string(n_cases) + ": the table does not tile the text"); continue; }
            std::ostringstream got;
            for (const svt_tbx_line& l : r.lines)
                got << l.off << "," << l.len << "," << l.beg << "," << l.end << "," << l.chrom_len << "," << l.flags << ";";
            n_lines += r.lines.size();
            if ((got.str().empty() ? std::string("-") : got.str()) != want_rows) failed("case " + std::to_string(n_cases) + ": rows " + got.str());
            if (want_sorted == "!") {
                if (!r.bad_line) failed("case " + std::to_string(n_cases) + ": sorted what is not sortable");
            } else if (r.bad_line || r.sorted != unhex(want_sorted)) failed("case " + std::to_string(n_cases) + ": the sorted text differs");
        } else if (kind == "P") {
            for (size_t cut = 0; cut <= text.size(); ++cut) {
                ++n_prefixes;
                if (!run(std::vector<uint8_t>(text.begin(), text.begin() + cut), r)) failed("a prefix of " + std::to_string(cut) + " bytes");
            }
        }
    }
    std::cout << n_cases << " cases, " << n_lines << " lines, " << n_prefixes << " prefixes\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

// asan_vcf_group_main.cpp -- svtyper_amd/csrc/svt_vcf_group.h (the per-line rule, the host twin of the scan kernel, the plain C++
// of the marked lines, the join and the writer) compiled into a stand-alone program with -fsanitize=address,undefined
// (tests/test_group_native.py).  Every text and every table lies in a heap buffer of exactly its length: no slack behind it.
//
// Input, one case per line:
//   C <samples> <format table hex> <info table hex> <text hex> <output hex> <!line,kind or ->
//   P <samples> <format table hex> <info table hex> <line hex>      every prefix of the line
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_vcf_lines.h"
#include "svt_vcf_group.h"

namespace group = svt::group;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& bytes)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[bytes.size()]);
    for (size_t i = 0; i < bytes.size(); ++i) p[i] = bytes[i];
    return p;
}

static int failures = 0;
static void failed(const std::string& what)
{
    std::cout << "FAILED " << what << "\n";
    ++failures;
}

struct Tables {
    uint32_t n_samples = 0;
    std::vector<uint8_t> formats, infos;
};

// one body through group_host and write_plan: "<output hex> <!line,kind or ->"
static std::string body(const std::vector<uint8_t>& bytes, size_t len, const Tables& t, uint64_t& host_lines)
{
    const std::vector<uint8_t> cut(bytes.begin(), bytes.begin() + (long)len);
    auto text = exact(cut), formats = exact(t.formats);
    uint64_t lines_in_text = 0;
    for (uint8_t c : cut) lines_in_text += c == '\n';
    lines_in_text += !cut.empty() && cut.back() != '\n';
    std::vector<svt_group_line> lines(lines_in_text + 1);
    std::vector<svt_group_out> plan(2 * lines_in_text + 2);
    svt_group_report report;
    uint64_t n_lines = 0, n_plan = 0;
    group::Block b;
    if (const char* why = group::take_arguments(text.get(), len, t.n_samples, formats.get(), t.formats.size(), lines.data(), &n_lines, plan.data(),
                                                &n_plan, &report, b))
        return std::string("?") + why;
    if (const char* why = group::group_host(b, lines.data(), lines_in_text, &n_lines, plan.data(), &n_plan, report)) return std::string("?") + why;
    if (n_lines != lines_in_text || n_plan > 2 * n_lines) return "?lines";
    host_lines += report.host_lines;
    group::Block w;
    if (!svt::cohort::parse_format_table(t.formats.data(), t.formats.size(), w.formats) ||
        !svt::cohort::parse_info_table(t.infos.data(), t.infos.size(), w.info))
        return "?tables";
    w.text = text.get();
    w.len = len;
    w.pr.n_samples = t.n_samples;
    std::vector<uint64_t> out_off(n_plan + 1);
    std::string out;
    svt_group_report written = svt_group_report();
    if (const char* why = group::write_plan(w, lines.data(), n_lines, plan.data(), n_plan, out_off.data(), out, written)) return std::string("?") + why;
    if (written.bad_line) return "?an entry of the plan cannot be written";
    if (out_off[n_plan] != out.size()) return "?offsets";
    static const char digits[] = "0123456789abcdef";
    std::string hex;
    for (unsigned char c : out) {
        hex += digits[c >> 4];
        hex += digits[c & 15];
    }
    if (hex.empty()) hex = "-";
    return hex + " " + (report.bad_line ? "!" + std::to_string(report.bad_line) + "," + std::to_string(report.bad_kind) : std::string("-"));
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t cases = 0, prefixes = 0, host_lines = 0, unused = 0;
    while (std::getline(in, row)) {
        std::istringstream f(row);
        std::string kind, formats, infos, text, want, death;
        Tables t;
        f >> kind >> t.n_samples >> formats >> infos;
        t.formats = unhex(formats);
        t.infos = unhex(infos);
        if (kind == "C") {
            f >> text >> want >> death;
            const std::vector<uint8_t> bytes = unhex(text);
            const std::string got = body(bytes, bytes.size(), t, host_lines);
            if (got != want + " " + death) failed("case " + std::to_string(cases) + ": " + got.substr(0, 200) + " for " + want.substr(0, 200) + " " + death);
            ++cases;
        } else if (kind == "P") {
            f >> text;
            const std::vector<uint8_t> bytes = unhex(text);
            for (size_t k = 0; k <= bytes.size(); ++k) {
                const std::string got = body(bytes, k, t, unused);
                if (!got.empty() && got[0] == '?') failed("prefix " + std::to_string(k) + ": " + got);
                ++prefixes;
            }
        }
    }
    std::cout << "cases " << cases << " prefixes " << prefixes << " host_lines " << host_lines << "\n";
    return failures ? 1 : 0;
}

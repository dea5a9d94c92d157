// asan_vcf_update_info_main.cpp -- svtyper_amd/csrc/svt_vcf_update_info.h (the per-line rule, the host twin of the kernel, the plain
// C++ of the marked lines and the writer) compiled into a stand-alone program with -fsanitize=address,undefined
// (tests/test_update_info_native.py).  Every text and every table lies in a heap buffer of exactly its length: no slack behind it.
//
// Input, one case per line:
//   C <samples> <format table hex> <info table hex> <text hex> <output hex, or !line,kind>
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
#include "svt_vcf_update_info.h"

namespace update_info = svt::update_info;

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

// one block through update_info_host and write_block; the output, or "!line,kind"
static std::string block(const std::vector<uint8_t>& bytes, size_t len, const Tables& t, uint64_t& host_lines)
{
    const std::vector<uint8_t> cut(bytes.begin(), bytes.begin() + (long)len);
    auto text = exact(cut), formats = exact(t.formats);
    uint64_t lines_in_text = 0;
    for (uint8_t c : cut) lines_in_text += c == '\n';
    lines_in_text += !cut.empty() && cut.back() != '\n';
    std::vector<svt_update_info_line> results(lines_in_text + 1);
    svt_update_info_report info;
    uint64_t n_lines = 0;
    update_info::Block b;
    if (const char* why = update_info::take_arguments(text.get(), len, t.n_samples, formats.get(), t.formats.size(), results.data(), &n_lines, &info, b))
        return std::string("?") + why;
    std::vector<svt_tbx_line> table;
    if (const char* why = update_info::update_info_host(b, table, results.data(), lines_in_text, &n_lines, info)) return std::string("?") + why;
    if (n_lines != lines_in_text) return "?lines";
    host_lines += info.host_lines;
    if (info.bad_line) return "!" + std::to_string(info.bad_line) + "," + std::to_string(info.bad_kind);
    update_info::Block w;
    if (!svt::cohort::parse_format_table(t.formats.data(), t.formats.size(), w.formats) ||
        !svt::cohort::parse_info_table(t.infos.data(), t.infos.size(), w.info))
        return "?tables";
    w.text = text.get();
    w.len = len;
    w.pr.n_samples = t.n_samples;
    std::vector<uint64_t> out_off(n_lines + 1);
    std::string out;
    svt_update_info_report written = svt_update_info_report();
    if (const char* why = update_info::write_block(w, table, results.data(), n_lines, out_off.data(), out, written)) return std::string("?") + why;
    if (written.bad_line) return "!" + std::to_string(written.bad_line) + "," + std::to_string(written.bad_kind);
    if (out_off[n_lines] != out.size()) return "?offsets";
    static const char digits[] = "0123456789abcdef";
    std::string hex;
    for (unsigned char c : out) {
        hex += digits[c >> 4];
        hex += digits[c & 15];
    }
    return hex.empty() ? "-" : hex;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t cases = 0, prefixes = 0, host_lines = 0, unused = 0;
    while (std::getline(in, row)) {
        std::istringstream f(row);
        std::string kind, formats, infos, text, want;
        Tables t;
        f >> kind >> t.n_samples >> formats >> infos;
        t.formats = unhex(formats);
        t.infos = unhex(infos);
        if (kind == "C") {
            f >> text >> want;
            const std::vector<uint8_t> bytes = unhex(text);
            const std::string got = block(bytes, bytes.size(), t, host_lines);
            if (got != want) failed("case " + std::to_string(cases) + ": " + got.substr(0, 200) + " for " + want.substr(0, 200));
            ++cases;
        } else if (kind == "P") {
            f >> text;
            const std::vector<uint8_t> bytes = unhex(text);
            for (size_t k = 0; k <= bytes.size(); ++k) {
                const std::string got = block(bytes, k, t, unused);
                if (!got.empty() && got[0] == '?') failed("prefix " + std::to_string(k) + ": " + got);
                ++prefixes;
            }
        }
    }
    std::cout << "cases " << cases << " prefixes " << prefixes << " host_lines " << host_lines << "\n";
    return failures ? 1 : 0;
}

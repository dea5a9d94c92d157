// asan_vcf_paste_main.cpp -- svtyper_amd/csrc/svt_vcf_paste.h (the per-line rule, the host twin of the kernels, the slow path and
// the builder of the first columns) compiled into a stand-alone program with -fsanitize=address,undefined
// (tests/test_paste_native.py).  Every text lies in a heap buffer of exactly its length: no slack behind it; the output in a
// buffer of exactly the size the call reports.
//
// Input, one case per line:  C <flags> <inputs> <lines> <info table hex> <text hex> <output hex, or !line,file,kind>   one block
//                            P <flags> <info table hex> <line hex>     every prefix of the line as a master's and an input's line
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_vcf_lines.h"
#include "svt_vcf_paste.h"

namespace paste = svt::paste;

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

// one block through paste_host, text and output in buffers of their own; the output, or "!line,file,kind"
static bool block(const std::vector<uint8_t>& bytes, uint32_t flags, uint32_t n_inputs, uint64_t n_lines, const std::vector<uint8_t>& table,
                  std::vector<uint8_t>& out, std::string& refusal, uint64_t& host_lines)
{
    std::unique_ptr<uint8_t[]> text(new uint8_t[bytes.size()]);
    for (size_t i = 0; i < bytes.size(); ++i) text[i] = bytes[i];
    std::unique_ptr<uint8_t[]> info_table(new uint8_t[table.size()]);
    for (size_t i = 0; i < table.size(); ++i) info_table[i] = table[i];
    std::vector<uint64_t> first(n_inputs + 1);
    for (uint32_t f = 0; f <= n_inputs; ++f) first[f] = f * n_lines;
    std::vector<svt_paste_line> results(n_lines ? n_lines : 1);
    svt_paste_info info;
    paste::Block b;
    std::unique_ptr<uint8_t[]> none(new uint8_t[1]);
    if (const char* why = paste::take_arguments(text.get(), bytes.size(), first.data(), n_inputs, n_lines, flags, info_table.get(), table.size(), none.get(),
                                                results.data(), &info, b)) {
        refusal = why;
        return false;
    }
    std::vector<svt_tbx_line> lines;
    // first for the size alone, then into a buffer of exactly that size
    const char* why = paste::paste_host(b, lines, results.data(), none.get(), 0, info);
    refusal.clear();
    out.clear();
    if (info.bad_line) {
        refusal = "!" + std::to_string(info.bad_line) + "," + std::to_string(info.bad_file) + "," + std::to_string(info.bad_kind);
        return true;
    }
    if (why && info.out_len == 0) {
        refusal = why;
        return false;
    }
    std::unique_ptr<uint8_t[]> exact(new uint8_t[info.out_len]);
    const uint64_t size = info.out_len;
    info = svt_paste_info();
    if ((why = paste::paste_host(b, lines, results.data(), exact.get(), size, info)) || info.out_len != size) {
        refusal = why ? why : "the two calls disagree about the size";
        return false;
    }
    uint64_t sum = 0;
    for (uint64_t j = 0; j < n_lines; ++j) sum += results[j].line_len;
    if (sum != size) {
        refusal = "the lines' sizes do not sum to the output's";
        return false;
    }
    host_lines = info.host_lines;
    out.assign(exact.get(), exact.get() + size);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_prefixes = 0, n_host = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind;
        fields >> kind;
        if (kind == "C") {
            uint32_t flags, n_inputs;
            uint64_t n_lines;
            std::string table_hex, text_hex, want;
            fields >> flags >> n_inputs >> n_lines >> table_hex >> text_hex >> want;
            ++n_cases;
            std::vector<uint8_t> out;
            std::string refusal;
            uint64_t host_lines = 0;
            if (!block(unhex(text_hex), flags, n_inputs, n_lines, unhex(table_hex), out, refusal, host_lines)) {
                failed("case " + std::to_string(n_cases) + ": " + refusal);
                continue;
            }
            n_host += host_lines;
            if (want[0] == '!') {
                if (refusal != want) failed("case " + std::to_string(n_cases) + ": " + (refusal.empty() ? "not refused" : refusal) + ", expected " + want);
            } else if (!refusal.empty() || out != unhex(want)) failed("case " + std::to_string(n_cases) + ": other bytes " + refusal);
        } else if (kind == "P") {
            uint32_t flags;
            std::string table_hex, line_hex;
            fields >> flags >> table_hex >> line_hex;
            const std::vector<uint8_t> line = unhex(line_hex), table = unhex(table_hex);
            for (size_t cut = 0; cut <= line.size(); ++cut) {
                ++n_prefixes;
                // the prefix with a newline as the master's line and as the one input's; then with the whole line as the master's
                for (int whole_master = 0; whole_master < 2; ++whole_master) {
                    std::vector<uint8_t> text;
                    if (whole_master) text.assign(line.begin(), line.end());
                    else text.assign(line.begin(), line.begin() + cut);
                    text.push_back('\n');
                    text.insert(text.end(), line.begin(), line.begin() + cut);
                    text.push_back('\n');
                    std::vector<uint8_t> out;
                    std::string refusal;
                    uint64_t host_lines = 0;
                    if (!block(text, flags, 1, 1, table, out, refusal, host_lines)) failed("a prefix of " + std::to_string(cut) + " bytes: " + refusal);
                }
                // the rule on the prefix without a newline, in a buffer that ends with it
                std::unique_ptr<uint8_t[]> bare(new uint8_t[cut]);
                for (size_t i = 0; i < cut; ++i) bare[i] = line[i];
                paste::Master m;
                paste::measure_master(bare.get(), cut, flags, m);
                paste::Input input;
                paste::measure_input(bare.get(), cut, bare.get(), m, flags | SVT_PASTE_SAFE, input);
                if (input.part_len && (uint64_t)input.part_b + input.part_len > cut) failed("a part beyond its line");
            }
        }
    }
    std::cout << "cases " << n_cases << " prefixes " << n_prefixes << " host_lines " << n_host << "\n";
    return failures ? 1 : 0;
}

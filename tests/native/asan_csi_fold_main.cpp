// asan_csi_fold_main.cpp -- the generalised index fold (svtyper_amd/csrc/svt_tbx_index.h: tbx::Contig in a scheme (14, depth), the
// .tbi serialiser and the CSIv1 one; svt_bai_index.h: the BAM's fold with the .bai serialiser and the CSIv1 one) compiled into a
// stand-alone program with -fsanitize=address,undefined (tests/test_csi_fold_native.py).  Every table lies in a heap buffer of
// exactly its length: no slack behind it.
//
// Input, one case per line:
//   B <n_ref> <l_ref_max> <rows "off,len,key,tid,beg,end,flags;..." or -> <member_start "a,b,..."> <member_off "a,b,...">
//     <expected .csi as hex, or !bad,kind>       the BAM fold as CSI over the table, compared; then as .bai and as CSI over the table
//                                                truncated at every length
//   V <payload> <text hex or -> <member_off "a,b,..."> <expected .csi as hex, or !bad,kind>
//                                                the line table of the text, the VCF fold as CSI, compared; then as .tbi and as CSI
//                                                over the table truncated at every length
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_bai_index.h"
#include "svt_tbx_index.h"

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto nibble = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : (c | 32) - 'a' + 10); };
    out.reserve(h.size() / 2);
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(nibble(h[i]) << 4 | nibble(h[i + 1])));
    return out;
}

static std::string hex(const std::vector<uint8_t>& bytes)
{
    static const char digits[] = "0123456789abcdef";
    std::string out;
    out.reserve(bytes.size() * 2);
    for (uint8_t b : bytes) {
        out.push_back(digits[b >> 4]);
        out.push_back(digits[b & 15]);
    }
    return out;
}

static std::vector<uint64_t> numbers(const std::string& text, char sep)
{
    std::vector<uint64_t> out;
    if (text == "-") return out;
    std::istringstream parts(text);
    std::string one;
    while (std::getline(parts, one, sep))
        if (!one.empty()) out.push_back(std::stoull(one));
    return out;
}

static int failures = 0;
static void failed(const std::string& what)
{
    std::cout << "FAILED " << what << "\n";
    ++failures;
}

static std::string outcome(uint64_t bad, uint32_t kind, const std::vector<uint8_t>& bytes)
{
    return bad ? "!" + std::to_string(bad) + "," + std::to_string(kind) : hex(bytes);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_folds = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind;
        fields >> kind;
        ++n_cases;
        if (kind == "B") {
            std::string n_ref_text, l_ref_text, rows, starts, offs, want;
            fields >> n_ref_text >> l_ref_text >> rows >> starts >> offs >> want;
            const int32_t n_ref = (int32_t)std::stol(n_ref_text);
            const uint64_t l_ref_max = std::stoull(l_ref_text);
            std::vector<svt_bam_span> table;
            if (rows != "-") {
                std::istringstream parts(rows);
                std::string one;
                while (std::getline(parts, one, ';')) {
                    const std::vector<uint64_t> v = numbers(one, ',');
                    if (v.size() != 7) return 3;
                    table.push_back(svt_bam_span{v[0], v[1], v[2], (int32_t)(int64_t)v[3], (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6]});
                }
            }
            const std::vector<uint64_t> member_start = numbers(starts, ','), member_off = numbers(offs, ',');
            if (member_start.empty() || member_start.size() != member_off.size()) return 3;
            for (uint64_t n = 0; n <= table.size(); ++n) {              // the table cut at every length, each in a buffer of its own
                std::unique_ptr<svt_bam_span[]> cut(new svt_bam_span[n]);
                for (uint64_t i = 0; i < n; ++i) cut[i] = table[i];
                std::unique_ptr<uint64_t[]> ms(new uint64_t[member_start.size()]), mo(new uint64_t[member_off.size()]);
                for (size_t k = 0; k < member_start.size(); ++k) { ms[k] = member_start[k]; mo[k] = member_off[k]; }
                std::vector<uint8_t> csi, bai;
                uint32_t why = 0;
                const uint64_t bad = svt::bai::build(cut.get(), n, n_ref, ms.get(), mo.get(), member_start.size() - 1, csi, why, true, l_ref_max);
                uint32_t why_bai = 0;
                (void)svt::bai::build(cut.get(), n, n_ref, ms.get(), mo.get(), member_start.size() - 1, bai, why_bai);
                n_folds += 2;
                if (n == table.size() && outcome(bad, why, csi) != want) failed("case " + std::to_string(n_cases) + ": " + outcome(bad, why, csi).substr(0, 200));
            }
        } else if (kind == "V") {
            std::string payload_text, text_hex, offs, want;
            fields >> payload_text >> text_hex >> offs >> want;
            const uint32_t payload = (uint32_t)std::stoul(payload_text);
            const std::vector<uint8_t> bytes = unhex(text_hex);
            std::unique_ptr<uint8_t[]> text(new uint8_t[bytes.size()]);
            for (size_t i = 0; i < bytes.size(); ++i) text[i] = bytes[i];
            const uint64_t n_lines = svt::tbx::count_lines(text.get(), bytes.size());
            std::vector<svt_tbx_line> lines(n_lines);
            svt::tbx::lines_host(text.get(), bytes.size(), lines.data());
            const std::vector<uint64_t> member_off = numbers(offs, ',');
            if (member_off.empty()) return 3;
            for (uint64_t n = 0; n <= n_lines; ++n) {
                std::unique_ptr<svt_tbx_line[]> cut(new svt_tbx_line[n]);
                for (uint64_t i = 0; i < n; ++i) cut[i] = lines[i];
                std::vector<uint8_t> csi, tbi;
                uint32_t why = 0, why_tbi = 0;
                const uint64_t bad = svt::tbx::build(text.get(), nullptr, cut.get(), n, bytes.size(), member_off.data(), member_off.size() - 1, payload, csi, why, true);
                (void)svt::tbx::build(text.get(), nullptr, cut.get(), n, bytes.size(), member_off.data(), member_off.size() - 1, payload, tbi, why_tbi);
                n_folds += 2;
                if (n == n_lines && outcome(bad, why, csi) != want) failed("case " + std::to_string(n_cases) + ": " + outcome(bad, why, csi).substr(0, 200));
            }
        } else {
            return 3;
        }
    }
    std::cout << n_cases << " cases, " << n_folds << " folds\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

// asan_bcf_main.cpp -- svtyper_amd/csrc/svt_bcf.h (the dictionaries, the record rule, the host twin) compiled into a stand-alone
// program with -fsanitize=address,undefined (tests/test_bcf_native.py).  Every text lies in a heap buffer of exactly its length:
// no slack behind it; every record is written into a buffer of exactly its measured size.
//
// Input, one case per line:  H <header hex>        the dictionaries the P rows are encoded against
//                            T <text hex> <flags> <stream hex, or !line,kind>    the whole text through encode_host
//                            P <line hex>          every prefix of the line through both walks, by strtod and by the exact rule
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_bcf.h"

namespace bcf = svt::bcf;

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

// both walks over the line `bytes`, in a buffer of its own; false where they disagree
static bool walks(const bcf::Dict& d, const std::vector<uint8_t>& bytes, bool exact)
{
    std::unique_ptr<uint8_t[]> line(new uint8_t[bytes.size()]);
    for (size_t i = 0; i < bytes.size(); ++i) line[i] = bytes[i];
    bcf::Sink count{nullptr, 0, 0};
    bcf::Measure m;
    if (bcf::encode_line(d, line.get(), bytes.size(), exact, count, m)) return m.at <= bytes.size();
    const uint64_t size = bcf::record_bytes(m);
    std::unique_ptr<uint8_t[]> record(new uint8_t[size]);
    bcf::Sink store{record.get(), size, 0};
    return bcf::encode_line(d, line.get(), bytes.size(), exact, store, m) == 0 && store.n == size;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_prefixes = 0, n_records = 0;
    bcf::Tables tables;
    std::unique_ptr<uint8_t[]> header;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind, text_hex, flags, want;
        fields >> kind >> text_hex >> flags >> want;
        const std::vector<uint8_t> text = unhex(text_hex);
        if (kind == "H") {
            header.reset(new uint8_t[text.size()]);
            for (size_t i = 0; i < text.size(); ++i) header[i] = text[i];
            if (const char* why = bcf::make_tables(header.get(), text.size(), tables)) failed(std::string("the header: ") + why);
        } else if (kind == "T") {
            ++n_cases;
            std::unique_ptr<uint8_t[]> buf(new uint8_t[text.size()]);
            for (size_t i = 0; i < text.size(); ++i) buf[i] = text[i];
            const uint32_t f = (uint32_t)std::stoul(flags);
            svt_bcf_info info = svt_bcf_info();
            bcf::Held held;
            if (const char* why = bcf::encode_host(buf.get(), text.size(), (f & SVT_BCF_SORT) != 0, (f & SVT_BCF_EXACT_FLOATS) != 0, info, held)) {
                failed("case " + std::to_string(n_cases) + ": " + why);
                continue;
            }
            if (want[0] == '!') {
                if ("!" + std::to_string(info.bad_line) + "," + std::to_string(info.bad_kind) != want)
                    failed("case " + std::to_string(n_cases) + ": refused line " + std::to_string(info.bad_line) + " kind " + std::to_string(info.bad_kind));
            } else if (info.bad_line || held.bytes != unhex(want)) failed("case " + std::to_string(n_cases) + ": the stream differs");
            n_records += info.n_records;
        } else if (kind == "P") {
            const bcf::Dict d = tables.view();
            for (size_t cut = 0; cut <= text.size(); ++cut) {
                ++n_prefixes;
                const std::vector<uint8_t> prefix(text.begin(), text.begin() + cut);
                if (!walks(d, prefix, false) || !walks(d, prefix, true)) failed("a prefix of " + std::to_string(cut) + " bytes of " + text_hex.substr(0, 60));
            }
        }
    }
    std::cout << n_cases << " cases, " << n_records << " records, " << n_prefixes << " prefixes\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

// asan_bcf_text_main.cpp -- svtyper_amd/csrc/svt_bcf_text.h (the dictionaries by index, the record rule, the host twin) compiled
// into a stand-alone program with -fsanitize=address,undefined (tests/test_bcf_text_native.py).  Every stream and every record
// lies in a heap buffer of exactly its length: no slack behind it; every line is written into a buffer of exactly its measured size.
//
// Input, one case per line:  S <stream hex> <flags> <block_bytes> <text hex, or !record,kind>    the whole stream through text_host
//                            M <stream hex>    every record of the stream, cut and changed, through both walks, by snprintf and by
//                                              the exact rule: every prefix as it is; every prefix from 8 bytes on with the two
//                                              lengths set to what is left (the shared part first); every byte (every seventh of a
//                                              record above 4096 bytes) set to six other values
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_bcf_text.h"

namespace bt = svt::bcftext;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

static int failures = 0;
static uint64_t n_walks = 0, n_lines = 0;
static void failed(const std::string& what)
{
    std::cout << "FAILED " << what << "\n";
    ++failures;
}

// both walks over the record `bytes`, in a buffer of its own: a refusal of a known kind, or a line both walks agree on
static bool walks(const bt::TextDict& d, const std::vector<uint8_t>& bytes, bool exact)
{
    ++n_walks;
    std::unique_ptr<uint8_t[]> rec(new uint8_t[bytes.size()]);
    for (size_t i = 0; i < bytes.size(); ++i) rec[i] = bytes[i];
    svt::bcf::Sink count{nullptr, 0, 0};
    bt::Shape sh;
    if (const uint32_t kind = bt::line_text(d, rec.get(), bytes.size(), exact, count, sh)) return kind >= 1 && kind <= 7;
    std::unique_ptr<uint8_t[]> line(new uint8_t[count.n]);
    svt::bcf::Sink store{line.get(), count.n, 0};
    bt::Shape again;
    ++n_lines;
    return bt::line_text(d, rec.get(), bytes.size(), exact, store, again) == 0 && store.n == count.n && count.n && line[count.n - 1] == '\n';
}

static void put32(std::vector<uint8_t>& b, size_t at, uint32_t v)
{
    for (int i = 0; i < 4; ++i) b[at + i] = (uint8_t)(v >> 8 * i);
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind, hex, flags, block, want;
        fields >> kind >> hex >> flags >> block >> want;
        const std::vector<uint8_t> bytes = unhex(hex);
        std::unique_ptr<uint8_t[]> stream(new uint8_t[bytes.size()]);
        for (size_t i = 0; i < bytes.size(); ++i) stream[i] = bytes[i];
        ++n_cases;
        const std::string name = "case " + std::to_string(n_cases);
        if (kind == "S") {
            svt_bcf_text_info info = svt_bcf_text_info();
            bt::TextHeld held;
            if (const char* why = bt::text_host(stream.get(), bytes.size(), std::stoul(flags) != 0, std::stoull(block), info, held)) {
                if (want != std::string("?") + why) failed(name + ": " + why);
                continue;
            }
            if (want[0] == '!') {
                if ("!" + std::to_string(info.bad_record) + "," + std::to_string(info.bad_kind) != want)
                    failed(name + ": refused record " + std::to_string(info.bad_record) + " kind " + std::to_string(info.bad_kind) + ", not " + want);
            } else if (info.bad_record || held.text != unhex(want)) failed(name + ": the text differs");
        } else if (kind == "M") {
            bt::TextTables t;
            uint64_t body = 0;
            if (const char* why = bt::read_stream_header(stream.get(), bytes.size(), t, body)) {
                failed(name + ": " + why);
                continue;
            }
            const bt::TextDict d = t.view();
            std::vector<uint64_t> chain;
            if (bt::walk_chain(stream.get(), bytes.size(), body, chain)) failed(name + ": the chain is cut short");
            static const uint8_t kValues[6] = {0x00, 0x01, 0x7F, 0x80, 0xF7, 0xFF};
            for (size_t j = 0; j + 1 < chain.size(); ++j) {
                const std::vector<uint8_t> rec(bytes.begin() + chain[j], bytes.begin() + chain[j + 1]);
                const uint32_t ls = bt::load32(rec.data(), 8, 0);
                bool ok = walks(d, rec, false) && walks(d, rec, true);
                for (size_t cut = 0; cut < rec.size(); ++cut) {
                    std::vector<uint8_t> prefix(rec.begin(), rec.begin() + cut);
                    ok = walks(d, prefix, false) && walks(d, prefix, true) && ok;
                    if (cut < 8) continue;
                    const uint32_t left = (uint32_t)cut - 8, shared = left < ls ? left : ls;
                    put32(prefix, 0, shared);
                    put32(prefix, 4, left - shared);
                    ok = walks(d, prefix, false) && walks(d, prefix, true) && ok;
                }
                for (size_t at = 0; at < rec.size(); at += rec.size() > 4096 ? 7 : 1)
                    for (uint8_t v : kValues) {
                        std::vector<uint8_t> changed = rec;
                        changed[at] = v == rec[at] ? (uint8_t)(v ^ 0x55) : v;
                        ok = walks(d, changed, false) && walks(d, changed, true) && ok;
                    }
                if (!ok) failed(name + ": record " + std::to_string(j + 1));
            }
        }
    }
    std::cout << n_cases << " cases, " << n_walks << " walks, " << n_lines << " lines\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

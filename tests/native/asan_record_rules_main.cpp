// The record rules (svtyper_amd/csrc/svt_record_rules.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
// program.  It reads tests/golden/record_grammar_areas.txt (written from tests/grammarcases.py): the tag areas of the grammar
// corpus with what grammarcases.spec_tags finds in them, two whole records and the CIGAR texts of the SA entries.  Every area,
// record and text is handed over as every one of its prefixes, each in a heap buffer of exactly that many bytes, so that a read
// one byte past the end is seen.  At full length the answer has to be the fixture's.
//
//   T <label> <stop_at_rg> <outcome> <at> <have_rg> <rg_off> <rg_len> <have_sa> <sa_off> <sa_len> <hex>
//   R <label> <tags_off> <hex>
//   C <text> <operations> <query> <clips> <ref>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "svt_record_rules.h"

namespace rr = svt::rr;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

// a heap copy of the first k bytes and nothing behind them
struct Prefix {
    uint8_t* p;
    Prefix(const std::vector<uint8_t>& all, size_t k) : p((uint8_t*)std::malloc(k ? k : 1)) { if (k) std::memcpy(p, all.data(), k); }
    ~Prefix() { std::free(p); }
};

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s record_grammar_areas.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned n_areas = 0, n_records = 0, n_cigars = 0, n_calls = 0;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string kind;
        f >> kind;
        if (kind == "T") {
            std::string label, outcome, hex;
            unsigned stop, at, have_rg, rg_off, rg_len, have_sa, sa_off, sa_len;
            f >> label >> stop >> outcome >> at >> have_rg >> rg_off >> rg_len >> have_sa >> sa_off >> sa_len >> hex;
            const std::vector<uint8_t> area = unhex(hex);
            const uint32_t want = outcome == "END" ? rr::TAGS_END : outcome == "AT_RG" ? rr::TAGS_AT_RG : rr::TAGS_MALFORMED;
            for (size_t k = 0; k <= area.size(); ++k) {
                Prefix buf(area, k);
                rr::Tags t;
                rr::tags_begin(t);
                uint32_t pos = 0;
                const uint32_t r = rr::walk_tags(buf.p, (uint32_t)k, pos, stop != 0, t);
                ++n_calls;
                CHECK(r == rr::TAGS_END || r == rr::TAGS_AT_RG || r == rr::TAGS_MALFORMED || r == rr::TAGS_OVERRUN, "%s k %zu: %u", label.c_str(), k, r);
                CHECK(pos <= k, "%s k %zu: at %u", label.c_str(), k, pos);
                CHECK(!t.have_rg || (uint64_t)t.rg_off + t.rg_len < k, "%s k %zu: RG value beyond the prefix", label.c_str(), k);
                CHECK(!t.have_sa || (uint64_t)t.sa_off + t.sa_len < k, "%s k %zu: SA value beyond the prefix", label.c_str(), k);
                CHECK(r != rr::TAGS_AT_RG || (stop && t.have_rg), "%s k %zu: AT_RG", label.c_str(), k);
                // what a prefix finds is what the whole area has there: nothing is found inside another tag's value
                if (t.have_rg && have_rg) CHECK(t.rg_off == rg_off && t.rg_len == rg_len, "%s k %zu: RG at %u+%u", label.c_str(), k, t.rg_off, t.rg_len);
                if (t.have_sa && have_sa) CHECK(t.sa_off == sa_off && t.sa_len == sa_len, "%s k %zu: SA at %u+%u", label.c_str(), k, t.sa_off, t.sa_len);
                CHECK(!(t.have_rg && !have_rg) && !(t.have_sa && !have_sa), "%s k %zu: found a tag the area does not have", label.c_str(), k);
                if (k < area.size()) continue;
                CHECK(r == want, "%s: outcome %u, expected %s", label.c_str(), r, outcome.c_str());
                if (want == rr::TAGS_MALFORMED) continue;
                CHECK(t.have_rg == (have_rg != 0) && t.have_sa == (have_sa != 0), "%s: have_rg %d have_sa %d", label.c_str(), t.have_rg, t.have_sa);
                if (want == rr::TAGS_AT_RG) CHECK(pos == at, "%s: at %u, expected %u", label.c_str(), pos, at);
                if (want == rr::TAGS_AT_RG && r == want) {          // the second leg ends the walk and adds the SA behind RG, if any
                    CHECK(rr::walk_tags(buf.p, (uint32_t)k, pos, false, t) == rr::TAGS_END, "%s: second leg", label.c_str());
                }
            }
            ++n_areas;
        } else if (kind == "R") {
            std::string label, hex;
            unsigned tags_off;
            f >> label >> tags_off >> hex;
            const std::vector<uint8_t> rec = unhex(hex);
            for (size_t k = 0; k <= rec.size(); ++k) {
                Prefix buf(rec, k);
                rr::Core c;
                const bool ok = rr::decode_core(buf.p, (uint32_t)k, c);
                ++n_calls;
                CHECK(!ok || c.tags_off <= k, "%s k %zu: tags_off %u", label.c_str(), k, c.tags_off);
                CHECK(ok == (k >= tags_off), "%s k %zu: %d", label.c_str(), k, (int)ok);
                if (ok) CHECK(c.tags_off == tags_off, "%s k %zu: tags_off %u", label.c_str(), k, c.tags_off);
            }
            ++n_records;
        } else if (kind == "C") {
            std::string text;
            unsigned ops;
            long long query, clips, ref;
            f >> text >> ops >> query >> clips >> ref;
            const std::vector<uint8_t> s(text.begin(), text.end());
            for (size_t k = 0; k <= s.size(); ++k) {
                Prefix buf(s, k);
                rr::CigarStats c;
                const uint32_t r = rr::cigar_of_string(buf.p, (uint32_t)k, 256, 15, c);
                ++n_calls;
                CHECK(r == rr::CIGAR_OK || r == rr::CIGAR_MALFORMED || r == rr::CIGAR_TOO_MANY, "%s k %zu: %u", text.c_str(), k, r);
                CHECK(c.n <= ops, "%s k %zu: %u operations", text.c_str(), k, c.n);
                if (k == s.size()) CHECK(r == rr::CIGAR_OK && c.n == ops && c.query == query && c.clips == clips && c.ref == ref, "%s: %u %u %lld %lld %lld",
                                         text.c_str(), r, c.n, (long long)c.query, (long long)c.clips, (long long)c.ref);
            }
            ++n_cigars;
        }
    }
    std::printf("%u tag areas, %u records, %u CIGAR texts, %u calls\n", n_areas, n_records, n_cigars, n_calls);
    if (failures || !n_areas || !n_records || !n_cigars) { std::printf("FAILED %d checks\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}

// asan_bam_first_main.cpp -- svtyper_amd/csrc/svt_bam_first_rules.h (the key of a record, key_equal, key_hash and the host twin of
// the whole pass) compiled into a stand-alone program with -fsanitize=address,undefined (tests/test_bam_first_native.py).
//
// Input, one case per line:  C <records hex, comma-separated, "." for an empty span, or -> <expected "k,k,..." (keep), - (no records)
//                              or !<bad record>>
// A case runs twice.  Once as a stream: the records side by side in a heap buffer of exactly their length, through
// bfr::first_host.  Once record by record: EVERY record in a heap buffer of its own that ends at the record's last byte, so a read
// past a record's span -- which inside the stream would land in its neighbour -- is caught; the keys of those copies are hashed,
// compared pair by pair (the device's walk: first occurrence = no equal key in front) and must give the same answer.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_bam_first_rules.h"

namespace bfr = svt::bfr;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "." || h == "-") return out;
    auto nibble = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : (c | 32) - 'a' + 10); };
    out.reserve(h.size() / 2);
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(nibble(h[i]) << 4 | nibble(h[i + 1])));
    return out;
}

static int failures = 0;
static void failed(const std::string& what)
{
    std::cout << "FAILED " << what << "\n";
    ++failures;
}

static std::string answer(const std::vector<uint8_t>& keep, uint64_t bad)
{
    std::ostringstream s;
    if (bad) s << "!" << bad;
    else
        for (size_t i = 0; i < keep.size(); ++i) s << (i ? "," : "") << (int)keep[i];
    return s.str().empty() ? "-" : s.str();
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_records = 0, n_bad = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind, hex, want;
        fields >> kind >> hex >> want;
        if (kind != "C") continue;
        ++n_cases;
        std::vector<std::vector<uint8_t>> records;
        if (hex != "-") {
            std::istringstream parts(hex);
            std::string one;
            while (std::getline(parts, one, ',')) records.push_back(unhex(one));
        }
        const uint64_t n = records.size();
        n_records += n;
        // the stream: exactly len bytes
        std::vector<uint64_t> rec_off(n + 1, 0);
        for (uint64_t i = 0; i < n; ++i) rec_off[i + 1] = rec_off[i] + records[i].size();
        const uint64_t len = rec_off[n];
        std::unique_ptr<uint8_t[]> stream(new uint8_t[len]);
        for (uint64_t i = 0; i < n; ++i)
            if (!records[i].empty()) std::memcpy(stream.get() + rec_off[i], records[i].data(), records[i].size());
        std::vector<uint8_t> keep(n, 9);
        uint64_t n_kept = 0;
        const uint64_t bad = bfr::first_host(stream.get(), len, rec_off.data(), n, keep.data(), n_kept);
        if (bad) ++n_bad;
        if (answer(keep, bad) != want) failed("case " + std::to_string(n_cases) + " as a stream: " + answer(keep, bad));
        if (!bad) {
            uint64_t sum = 0;
            for (uint8_t k : keep) sum += k;
            if (sum != n_kept) failed("case " + std::to_string(n_cases) + ": n_kept");
        }
        // record by record: a buffer each that ends at the record's last byte
        std::vector<std::unique_ptr<uint8_t[]>> own(n);
        std::vector<bfr::Key> keys(n);
        std::vector<uint64_t> hashes(n);
        std::vector<uint8_t> keep2(n, 9);
        uint64_t bad2 = 0;
        for (uint64_t i = 0; i < n && !bad2; ++i) {
            own[i].reset(new uint8_t[records[i].size()]);
            if (!records[i].empty()) std::memcpy(own[i].get(), records[i].data(), records[i].size());
            const uint64_t off[2] = {0, records[i].size()};
            if (!bfr::key_at(own[i].get(), records[i].size(), off, 0, keys[i])) {
                bad2 = i + 1;
                break;
            }
            hashes[i] = bfr::key_hash(keys[i]);
            keep2[i] = 1;
            for (uint64_t j = i; j > 0; --j) {
                const bool same = bfr::key_equal(keys[i], keys[j - 1]);
                if (same && hashes[i] != hashes[j - 1]) failed("case " + std::to_string(n_cases) + ": equal keys, two hashes");
                if (same) keep2[i] = 0;
            }
        }
        if (answer(keep2, bad2) != want) failed("case " + std::to_string(n_cases) + " record by record: " + answer(keep2, bad2));
        // masks of every width leave the low bits alone
        for (uint32_t bits = 1; bits <= 64; ++bits)
            if ((bfr::hash_mask(bits) & 1) != 1 || (bits < 64 && bfr::hash_mask(bits) >> bits)) failed("hash_mask " + std::to_string(bits));
    }
    std::cout << n_cases << " cases, " << n_records << " records, " << n_bad << " refused\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

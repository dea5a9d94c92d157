// asan_bam_sort_main.cpp -- svtyper_amd/csrc/svt_bam_sort_rules.h (the per-record rule, the host span table, the order, the member
// cut) and svt_bai_index.h (the index fold) compiled into a stand-alone program with -fsanitize=address,undefined
// (tests/test_bam_sort_native.py).  Every stream lies in a heap buffer of exactly its length: no slack behind it.
//
// Input, one case per line:  C <n_ref> <records hex, comma-separated, or -> <expected rows "off,len,key,tid,beg,end,flags;..." or ->
//                              <expected order "i,i,..." , - (no records) or ! (refused)>
//                            P <n_ref> <record hex> [<lo> <hi>]   every prefix of the record (of lo <= length < hi) through the table, the
//                              order and the fold
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_bai_index.h"
#include "svt_bam_sort_rules.h"

namespace bsr = svt::bsr;

static std::vector<uint8_t> unhex(const std::string& h)
{
    std::vector<uint8_t> out;
    if (h == "-") return out;
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

struct Run {
    std::vector<svt_bam_span> spans;
    std::vector<uint64_t> perm;
    uint64_t bad = 0;
    uint32_t kind = 0;
};

// the table, the order, the records in that order and the fold over both streams
static void run(const std::vector<std::vector<uint8_t>>& records, int32_t n_ref, Run& r)
{
    const uint64_t n = records.size();
    std::vector<uint64_t> rec_off(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) rec_off[i + 1] = rec_off[i] + records[i].size();
    const uint64_t len = rec_off[n];
    std::unique_ptr<uint8_t[]> stream(new uint8_t[len]);        // exactly len bytes
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t k = 0; k < records[i].size(); ++k) stream[rec_off[i] + k] = records[i][k];
    r.spans.assign(n, svt_bam_span());
    uint64_t key_and = 0, key_or = 0;
    bsr::spans_host(stream.get(), len, rec_off.data(), n, n_ref, r.spans.data(), key_and, key_or);
    auto fold = [&](const std::vector<svt_bam_span>& written) {
        if (n_ref > (1 << 20)) return;              // (the sort's case with reference ids up to 2^30: an index has a slot per reference)
        std::vector<uint64_t> start, off;
        bsr::cut_members(0, written.size(), [&](uint64_t j) { return written[j].len; }, start);
        for (uint64_t k = 0; k < start.size(); ++k) off.push_back(61 * k);
        std::vector<uint8_t> index;
        uint32_t kind = 0;
        (void)svt::bai::build(written.data(), written.size(), n_ref, start.data(), off.data(), start.size() - 1, index, kind);
    };
    fold(r.spans);
    r.perm.assign(n, 0);
    r.bad = bsr::sort_order(r.spans.data(), n, r.perm.data(), r.kind);
    if (r.bad) return;
    std::vector<svt_bam_span> written(n);
    std::unique_ptr<uint8_t[]> out(new uint8_t[len]);
    uint64_t at = 0;
    for (uint64_t j = 0; j < n; ++j) {
        written[j] = r.spans[r.perm[j]];
        for (uint64_t k = 0; k < written[j].len; ++k) out[at + k] = stream[written[j].off + k];
        written[j].off = at;
        at += written[j].len;
    }
    fold(written);
}

// one span of `cut` bytes in a heap buffer of exactly that size through the table, the order and the fold (what run() does for a
// stream of one record, without its vectors: this runs once per byte of the corpus); `claim`: block_size says the cut is whole
static uint32_t run_prefix(const uint8_t* record, uint64_t cut, bool claim, int32_t n_ref)
{
    std::unique_ptr<uint8_t[]> stream(new uint8_t[cut]);
    if (cut) std::memcpy(stream.get(), record, cut);
    if (claim)
        for (int k = 0; k < 4; ++k) stream[k] = (uint8_t)((cut - 4) >> (8 * k));
    const uint64_t rec_off[2] = {0, cut};
    svt_bam_span span;
    uint64_t key_and = 0, key_or = 0, perm = 0;
    bsr::spans_host(stream.get(), cut, rec_off, 1, n_ref, &span, key_and, key_or);
    uint32_t kind = 0;
    (void)bsr::sort_order(&span, 1, &perm, kind);
    if (n_ref <= (1 << 20)) {
        const uint64_t start[2] = {0, cut}, off[2] = {0, 61};
        std::vector<uint8_t> index;
        (void)svt::bai::build(&span, 1, n_ref, start, off, cut ? 1 : 0, index, kind);
    }
    return span.flags;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string row;
    uint64_t n_cases = 0, n_prefixes = 0, n_records = 0;
    while (std::getline(in, row)) {
        std::istringstream fields(row);
        std::string kind, n_ref_text, hex, want_rows, want_order;
        fields >> kind >> n_ref_text >> hex >> want_rows >> want_order;
        const int32_t n_ref = (int32_t)std::stol(n_ref_text);
        Run r;
        if (kind == "C") {
            ++n_cases;
            std::vector<std::vector<uint8_t>> records;
            if (hex != "-") {
                std::istringstream parts(hex);
                std::string one;
                while (std::getline(parts, one, ',')) records.push_back(unhex(one));
            }
            run(records, n_ref, r);
            n_records += records.size();
            std::ostringstream got, order;
            for (const svt_bam_span& s : r.spans)
                got << s.off << "," << s.len << "," << s.key << "," << s.tid << "," << s.beg << "," << s.end << "," << s.flags << ";";
            if ((got.str().empty() ? std::string("-") : got.str()) != want_rows) failed("case " + std::to_string(n_cases) + ": rows " + got.str());
            if (r.bad) order << "!" << r.bad << "," << r.kind;
            else
                for (uint64_t j = 0; j < r.perm.size(); ++j) order << (j ? "," : "") << r.perm[j];
            if ((order.str().empty() ? std::string("-") : order.str()) != want_order) failed("case " + std::to_string(n_cases) + ": order " + order.str());
        } else if (kind == "P") {
            const std::vector<uint8_t> record = unhex(hex);
            // (cuts [lo, hi) where the row names them: a long record's cuts are dealt to several runs of this program)
            const size_t lo = want_rows.empty() ? 0 : (size_t)std::stoull(want_rows);
            const size_t hi = want_order.empty() ? record.size() + 1 : (size_t)std::stoull(want_order);
            for (size_t cut = lo; cut < hi && cut <= record.size(); ++cut) {
                ++n_prefixes;
                const uint32_t flags = run_prefix(record.data(), cut, false, n_ref);
                // a proper prefix never is the whole record: its block_size says so, or there is no block_size
                if (cut < record.size() && !(flags & SVT_BAM_BAD)) failed("a prefix of " + std::to_string(cut) + " bytes was taken for a record");
                // the same prefix with a block_size that claims it is whole: the name and the CIGAR are what is cut short now
                if (cut >= 4) (void)run_prefix(record.data(), cut, true, n_ref);
            }
        }
    }
    std::cout << n_cases << " cases, " << n_records << " records, " << n_prefixes << " prefixes\n";
    std::cout << (failures ? "failed" : "ok") << "\n";
    return failures ? 1 : 0;
}

// The index model (svtyper_amd/csrc/svt_bam_index.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
// program: the header compiled alone with its own main, as tests/native/asan_record_rules_main.cpp runs the record rules.
//
//   asan_csi <clean.csi> [<broken.csi> ...]
//
// Every file is read into a heap buffer of exactly its size (a read one byte past the end is seen) and handed to
// svt::bamidx::load.  The first has to load, every other one has to be refused with a text that names it.  On the clean index
// 1 000 random windows then go through clip / reg2bins / min_offset / fetch_chunks: every bin has to be one of the scheme's and
// to overlap the window, no overlapping bin may be missing, min_offset has to be the loffset of a bin that starts at or below
// the window, and the merged chunks have to be ascending and apart.  The same windows go through an index of every scheme the
// tests use, and through record_starts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "svt_bam_index.h"

namespace bx = svt::bamidx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// the file's bytes in a heap block of exactly that size
struct Bytes {
    uint8_t* p = nullptr;
    size_t n = 0;
    explicit Bytes(const char* path)
    {
        FILE* f = std::fopen(path, "rb");
        if (!f) return;
        std::fseek(f, 0, SEEK_END);
        n = (size_t)std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        p = (uint8_t*)std::malloc(n ? n : 1);
        if (n && std::fread(p, 1, n, f) != n) n = 0;
        std::fclose(f);
    }
    ~Bytes() { std::free(p); }
};

// level and first position of a bin of the scheme
static void bin_span(const bx::Index& idx, uint32_t bin, int64_t& beg, int64_t& end)
{
    int l = 0;
    while (l < idx.depth && bx::Index::level_first(l + 1) <= bin) ++l;
    const int s = idx.level_shift(l);
    beg = (int64_t)(bin - bx::Index::level_first(l)) << s;
    end = beg + ((int64_t)1 << s);
}

static unsigned query(const bx::Index& idx, std::mt19937_64& rng, int64_t contig_length)
{
    std::vector<uint32_t> bins;
    std::vector<bx::Chunk> chunks, merged;
    const int64_t span = std::min<int64_t>(idx.max_pos(), contig_length);
    const int32_t tid = (int32_t)(rng() % (idx.refs.size() + 1)) - (rng() % 16 == 0 ? 1 : 0);      // (now and then out of range)
    int64_t beg = (int64_t)(rng() % (uint64_t)(span + 1000)) - 500;
    int64_t end = beg + (int64_t)(rng() % 3 == 0 ? rng() % (uint64_t)span : rng() % 2000);
    idx.fetch_chunks(tid, beg, end, contig_length, bins, chunks, merged);
    for (size_t i = 0; i < merged.size(); ++i) {
        CHECK(merged[i].first <= merged[i].second, "chunk %zu", i);
        if (i) CHECK(merged[i - 1].second < merged[i].first, "chunks %zu and %zu touch or overlap", i - 1, i);
    }
    if (tid < 0 || (size_t)tid >= idx.refs.size()) { CHECK(merged.empty(), "chunks for tid %d", tid); return 1; }
    const uint64_t min_off = idx.min_offset(tid, beg);
    if (idx.kind == bx::KIND_CSI && min_off != 0) {
        bool found = false;
        for (const auto& kv : idx.refs[(size_t)tid].loffset) {
            int64_t b0 = 0, b1 = 0;
            bin_span(idx, kv.first, b0, b1);
            if (kv.second == min_off && b0 <= std::max<int64_t>(beg, 0)) found = true;
        }
        CHECK(found, "min_offset %llu of %lld is no loffset of a bin at or below it", (unsigned long long)min_off, (long long)beg);
    }
    if (!idx.clip(beg, end, contig_length)) { CHECK(merged.empty(), "chunks for an empty window"); return 1; }
    idx.reg2bins(beg, end, bins);
    CHECK(!bins.empty() && bins[0] == 0, "the root is not first");
    size_t want = 0;
    for (int l = 0; l <= idx.depth; ++l) want += (size_t)(((end - 1) >> idx.level_shift(l)) - (beg >> idx.level_shift(l)) + 1);
    CHECK(bins.size() == want, "%zu bins, %zu levels' worth expected", bins.size(), want);
    for (size_t i = 0; i < bins.size(); i += 1 + bins.size() / 64) {
        int64_t b0 = 0, b1 = 0;
        CHECK(bins[i] < idx.pseudo_bin() - 1, "bin %u is not one of the scheme", bins[i]);
        bin_span(idx, bins[i], b0, b1);
        CHECK(b0 < end && b1 > beg, "bin %u [%lld, %lld) does not overlap [%lld, %lld)", bins[i], (long long)b0, (long long)b1, (long long)beg, (long long)end);
    }
    return 1;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s clean.csi [broken.csi ...]\n", argv[0]); return 2; }
    unsigned loaded = 0, refused = 0, queries = 0;
    bx::Index clean;
    {
        const Bytes b(argv[1]);
        std::string err;
        CHECK(b.p && bx::load(b.p, b.n, argv[1], clean, err), "%s does not load: %s", argv[1], err.c_str());
        CHECK(clean.kind == bx::KIND_CSI && !clean.refs.empty(), "kind %d", clean.kind);
        if (failures) return 1;
        ++loaded;
        // every prefix of the clean file: refused or (a prefix that ends between members, behind every count) loaded -- never a read out of bounds
        for (size_t k = 0; k < b.n; k += 1 + k / 97) {
            uint8_t* p = (uint8_t*)std::malloc(k ? k : 1);
            std::memcpy(p, b.p, k);
            bx::Index idx;
            std::string e;
            if (!bx::load(p, k, "prefix", idx, e)) CHECK(e.find("prefix") != std::string::npos, "prefix %zu: %s", k, e.c_str());
            std::free(p);
        }
    }
    for (int a = 2; a < argc; ++a) {
        const Bytes b(argv[a]);
        bx::Index idx;
        std::string err;
        CHECK(b.p != nullptr, "cannot read %s", argv[a]);
        const bool ok = b.p && bx::load(b.p, b.n, argv[a], idx, err);
        CHECK(!ok, "%s loads", argv[a]);
        CHECK(ok || err.find(argv[a]) != std::string::npos, "%s: the text does not name the file: %s", argv[a], err.c_str());
        CHECK(ok || idx.kind == bx::KIND_NONE, "%s: a refused index has a kind", argv[a]);
        if (!ok) ++refused;
    }
    std::mt19937_64 rng(20261018);
    for (int k = 0; k < 1000; ++k) queries += query(clean, rng, 100000);
    std::vector<uint64_t> cuts;
    clean.record_starts(0, cuts);
    CHECK(!cuts.empty(), "no record starts");
    for (size_t i = 1; i < cuts.size(); ++i) CHECK(cuts[i - 1] < cuts[i], "record starts not ascending at %zu", i);
    // the arithmetic alone, on every scheme the tests use and on the widest one the loader lets in
    const int shapes[][2] = {{14, 5}, {14, 6}, {16, 5}, {13, 6}, {10, 3}, {0, 0}, {32, 10}, {62, 0}};
    for (const auto& s : shapes) {
        bx::Index idx;
        idx.kind = bx::KIND_CSI;
        idx.min_shift = s[0];
        idx.depth = s[1];
        idx.refs.resize(2);
        idx.refs[0].loffset[0] = 7;
        for (int k = 0; k < 50; ++k) query(idx, rng, 2147483647);
    }
    std::printf("%u loaded, %u refused, %u queries\n", loaded, refused, queries);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}

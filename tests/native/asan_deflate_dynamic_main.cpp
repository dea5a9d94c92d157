// The dynamic-Huffman mode of the one-source BGZF compressor (svtyper_amd/csrc/svt_deflate.h, dfl::kDynamic) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.  It reads the lines
// tests/test_sanitizers_deflate_dynamic.py writes from tests/dynhuffcases.py:
//
//   P <payload hex | ->
//   H <limit> <frequency> <frequency> ...
//
// runs every histogram (the Fibonacci ones, whose trees are deeper than the limit, among them) through dfl::code_lengths, the
// frequencies and the lengths in heap buffers of exactly their size, and checks that the set is complete and within the limit;
// and then makes payloads of its own from a deterministic random stream (runs, copies from a little way back, noise: lengths
// 0 .. 65 280).  Every payload sits in a heap buffer of exactly its length, at every alignment mod 4, and is compressed into a
// heap buffer of exactly dfl::cdata_bound bytes: a read past the payload or a write past the bound is the sanitizer's to
// find.  Every output is inflated by svt_inflate.h and compared with the payload; the bytes must not depend on the alignment;
// a buffer one byte short of the bound is refused with nothing written; no output is longer than the fixed mode's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "svt_deflate.h"
#include "svt_inflate.h"

namespace dfl = svt::dfl;
namespace inf = svt::inf;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a heap block that ends exactly behind `n` bytes which begin `shift` bytes into it
struct Exact {
    uint8_t* base;
    uint8_t* p;
    Exact(size_t n, unsigned shift) : base((uint8_t*)std::malloc(n + shift ? n + shift : 1)), p(base + shift) {}
    ~Exact() { std::free(base); }
};

static std::unique_ptr<dfl::Scratch<1, dfl::kDynamic>> S(new dfl::Scratch<1, dfl::kDynamic>());
static std::unique_ptr<dfl::Scratch<1>> S0(new dfl::Scratch<1>());
static std::unique_ptr<inf::Scratch> I(new inf::Scratch());
static unsigned long long n_payloads = 0, n_bytes = 0, n_stored = 0, n_dynamic = 0, n_histograms = 0, n_deep = 0;

static void one(const std::vector<uint8_t>& payload, unsigned n_shifts)
{
    const uint32_t n = (uint32_t)payload.size(), bound = dfl::cdata_bound(n);
    std::vector<uint8_t> first;
    for (unsigned shift = 0; shift < n_shifts; ++shift) {
        Exact src(n, shift), dst(bound, (shift * 3) & 3);
        if (n) std::memcpy(src.p, payload.data(), n);
        std::memset(dst.p, 0xEE, bound);
        const uint32_t clen = dfl::deflate_member<dfl::HostCtx, dfl::kDynamic>(src.p, n, dst.p, bound, *S);
        CHECK(clen >= 2 && clen <= bound, "n %u: %u bytes, the bound is %u", n, clen, bound);
        if (clen < 2 || clen > bound) return;
        if (shift == 0) first.assign(dst.p, dst.p + clen);
        else CHECK(first.size() == clen && std::memcmp(first.data(), dst.p, clen) == 0, "n %u shift %u: the bytes depend on the alignment", n, shift);
        Exact cdata(clen, shift), back(n, (shift + 1) & 3);
        std::memcpy(cdata.p, dst.p, clen);
        const uint32_t st = inf::inflate_member<inf::HostCtx>(cdata.p, clen, back.p, n, *I);
        CHECK(st == inf::INF_OK, "n %u: svt_inflate.h answers %u", n, st);
        CHECK(st != inf::INF_OK || n == 0 || std::memcmp(back.p, payload.data(), n) == 0, "n %u: inflated bytes differ", n);
        if (shift == 0) {
            n_stored += n && clen == n + 5 && (dst.p[0] & 7) == 1;
            n_dynamic += (dst.p[0] & 7) == 5;
            Exact old(bound, 0);
            const uint32_t flen = dfl::deflate_member<dfl::HostCtx>(src.p, n, old.p, bound, *S0);
            CHECK(clen <= flen, "n %u: %u bytes, the fixed mode writes %u", n, clen, flen);
            CHECK((dst.p[0] & 7) == 5 ? clen < flen : clen == flen && std::memcmp(old.p, dst.p, clen) == 0, "n %u: not the fixed mode's bytes", n);
        }
    }
    {
        Exact src(n, 1), shorter(bound - 1, 0);
        if (n) std::memcpy(src.p, payload.data(), n);
        std::memset(shorter.p, 0xEE, bound - 1);
        CHECK((dfl::deflate_member<dfl::HostCtx, dfl::kDynamic>(src.p, n, shorter.p, bound - 1, *S)) == 0, "n %u: a short buffer is taken", n);
        bool clean = true;
        for (uint32_t i = 0; i + 1 < bound; ++i) clean = clean && shorter.p[i] == 0xEE;
        CHECK(clean, "n %u: a refused call wrote", n);
    }
    ++n_payloads;
    n_bytes += n;
}

// one histogram through the length builder: complete (or one code of one bit, or none), within the limit, a code where a
// frequency is and nowhere else
static void histogram(uint32_t limit, const std::vector<uint32_t>& freq)
{
    const uint32_t n = (uint32_t)freq.size();
    uint32_t* f = (uint32_t*)std::malloc(n * sizeof(uint32_t));
    uint8_t* len = (uint8_t*)std::malloc(n);
    std::memcpy(f, freq.data(), n * sizeof(uint32_t));
    std::memset(len, 0xEE, n);
    std::unique_ptr<dfl::Build> B(new dfl::Build());
    dfl::code_lengths<dfl::HostCtx>(f, n, limit, len, *B);
    uint64_t kraft = 0, used = 0, deepest = 0;
    for (uint32_t s = 0; s < n; ++s) {
        CHECK((len[s] != 0) == (f[s] != 0) && len[s] <= limit, "symbol %u: frequency %u, length %u", s, f[s], len[s]);
        if (len[s] && len[s] <= limit) { kraft += 1ull << (limit - len[s]); ++used; if (len[s] > deepest) deepest = len[s]; }
    }
    CHECK(used == 0 ? kraft == 0 : used == 1 ? kraft == 1ull << (limit - 1) : kraft == 1ull << limit, "%u symbols under %u: Kraft sum %llu", n, limit,
          (unsigned long long)kraft);
    n_deep += deepest == limit;
    ++n_histograms;
    std::free(f);
    std::free(len);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 24) % below);
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        if (line.size() >= 3 && line[0] == 'H') {
            std::istringstream fields(line.substr(2));
            uint32_t limit = 0, f;
            std::vector<uint32_t> freq;
            fields >> limit;
            while (fields >> f) freq.push_back(f);
            if ((limit == 7 || limit == 15) && !freq.empty() && freq.size() <= dfl::kLitSyms) histogram(limit, freq);
            continue;
        }
        if (line.size() < 3 || line[0] != 'P') continue;
        std::vector<uint8_t> payload;
        if (line[2] != '-')
            for (size_t i = 2; i + 1 < line.size(); i += 2) payload.push_back((uint8_t)std::strtoul(line.substr(i, 2).c_str(), nullptr, 16));
        one(payload, payload.size() <= 2048 ? 4 : 2);
    }
    const unsigned long long from_file = n_payloads;
    for (unsigned k = 0; k < 300; ++k) {
        const uint32_t n = k < 8 ? dfl::kMaxPayload - k : k < 200 ? rnd(3000) : rnd(dfl::kMaxPayload + 1);
        const uint32_t alphabet = 2 + rnd(255), back = 1 + rnd(2100);
        std::vector<uint8_t> payload;
        while (payload.size() < n) {
            const uint32_t kind = rnd(4), run = 1 + rnd(kind == 0 ? 600 : 40);
            for (uint32_t i = 0; i < run && payload.size() < n; ++i) {
                if (kind == 0 && payload.size() >= back) payload.push_back(payload[payload.size() - back]);     // a copy from `back` behind
                else if (kind == 1 && !payload.empty()) payload.push_back(payload.back());                       // a run
                else payload.push_back((uint8_t)(rnd(alphabet) + (kind == 3 ? 100 : 0)));
            }
        }
        one(payload, 2);
    }
    std::printf("%llu payloads, %llu from the file, %llu bytes, %llu stored, %llu dynamic, %llu histograms, %llu at the limit\n", n_payloads, from_file,
                n_bytes, n_stored, n_dynamic, n_histograms, n_deep);
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

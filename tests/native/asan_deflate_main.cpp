// The one-source BGZF compressor (svtyper_amd/csrc/svt_deflate.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
// stand-alone program.  It reads the lines tests/test_sanitizers_deflate.py writes from tests/deflatecases.py:
//
//   P <payload hex | ->
//
// and then makes payloads of its own from a deterministic random stream (runs, copies from a little way back, noise: lengths
// 0 .. 65 280).  Every payload sits in a heap buffer of exactly its length, at every alignment mod 4, and is compressed into a
// heap buffer of exactly dfl::cdata_bound bytes: a read past the payload or a write past the bound is the sanitizer's to
// find.  Every output is inflated by svt_inflate.h and compared with the payload; the bytes must not depend on the alignment;
// a buffer one byte short of the bound is refused with nothing written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
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

static std::unique_ptr<dfl::Scratch<1>> S(new dfl::Scratch<1>());
static std::unique_ptr<inf::Scratch> I(new inf::Scratch());
static unsigned long long n_payloads = 0, n_bytes = 0, n_stored = 0;

static void one(const std::vector<uint8_t>& payload, unsigned n_shifts)
{
    const uint32_t n = (uint32_t)payload.size(), bound = dfl::cdata_bound(n);
    std::vector<uint8_t> first;
    for (unsigned shift = 0; shift < n_shifts; ++shift) {
        Exact src(n, shift), dst(bound, (shift * 3) & 3);
        if (n) std::memcpy(src.p, payload.data(), n);
        std::memset(dst.p, 0xEE, bound);
        const uint32_t clen = dfl::deflate_member<dfl::HostCtx>(src.p, n, dst.p, bound, *S);
        CHECK(clen >= 2 && clen <= bound, "n %u: %u bytes, the bound is %u", n, clen, bound);
        if (clen < 2 || clen > bound) return;
        if (shift == 0) first.assign(dst.p, dst.p + clen);
        else CHECK(first.size() == clen && std::memcmp(first.data(), dst.p, clen) == 0, "n %u shift %u: the bytes depend on the alignment", n, shift);
        Exact cdata(clen, shift), back(n, (shift + 1) & 3);
        std::memcpy(cdata.p, dst.p, clen);
        const uint32_t st = inf::inflate_member<inf::HostCtx>(cdata.p, clen, back.p, n, *I);
        CHECK(st == inf::INF_OK, "n %u: svt_inflate.h answers %u", n, st);
        CHECK(st != inf::INF_OK || n == 0 || std::memcmp(back.p, payload.data(), n) == 0, "n %u: inflated bytes differ", n);
        if (shift == 0) n_stored += n && clen == n + 5 && (dst.p[0] & 7) == 1;
    }
    {
        Exact src(n, 1), shorter(bound - 1, 0);
        if (n) std::memcpy(src.p, payload.data(), n);
        std::memset(shorter.p, 0xEE, bound - 1);
        CHECK(dfl::deflate_member<dfl::HostCtx>(src.p, n, shorter.p, bound - 1, *S) == 0, "n %u: a short buffer is taken", n);
        bool clean = true;
        for (uint32_t i = 0; i + 1 < bound; ++i) clean = clean && shorter.p[i] == 0xEE;
        CHECK(clean, "n %u: a refused call wrote", n);
    }
    ++n_payloads;
    n_bytes += n;
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
    std::printf("%llu payloads, %llu from the file, %llu bytes, %llu stored\n", n_payloads, from_file, n_bytes, n_stored);
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

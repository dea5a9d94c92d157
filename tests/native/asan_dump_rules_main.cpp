// The dump rules (svtyper_amd/csrc/svt_dump_rules.h) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
// program.  It reads the lines tests/test_dump_rules_native.py writes from tests/dumpcases.py:
//
//   E <state> <record hex> <expected hex | ->
//
// one alignment record as it lies in a BAM (block_size first), a tag state (0 not set, 1 R, 2 A) and what bam.AlignmentFile.write
// emits for the read in that state -- or "-": the record is outside the dump's envelope.  Every record sits in a heap buffer of
// exactly its length, at every alignment mod 4, and is written into a heap buffer of exactly the expected length, at every
// alignment mod 4; the decision rule (size_fragment) has to find that length and that state.  Then every truncated prefix of
// the record, in a buffer of exactly its length, has to answer "outside the envelope" -- and, with its block_size word made to
// fit the prefix, whatever it answers, without a read past the end.  rr::tag_field has to walk a tag area as rr::walk_tags does.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "svt_dump_rules.h"

namespace dr = svt::dr;
namespace ew = svt::ew;
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

// a heap block that ends exactly behind `n` bytes which begin `shift` bytes into it (malloc aligns the block: p is `shift` mod 4)
struct Exact {
    uint8_t* base;
    uint8_t* p;
    Exact(size_t n, unsigned shift) : base((uint8_t*)std::malloc(n + shift ? n + shift : 1)), p(base + shift) {}
    Exact(const std::vector<uint8_t>& all, size_t n, unsigned shift) : Exact(n, shift) { if (n) std::memcpy(p, all.data(), n); }
    ~Exact() { std::free(base); }
};

// the fragment of one row whose only read is the record at offset 0, decided into `state`: a hit for R; for A a seq candidate
// (rec[2], verdict bit 16) or, with `clip`, a clip candidate (rec[3], bit 32) with p_alt > 0 -- and the other bit set on the row
// without its candidate is outside the envelope
static bool decide(const uint8_t* arena, uint64_t arena_len, unsigned state, uint32_t (&len)[2], uint8_t (&st)[2], bool clip = false, bool crossed = false)
{
    ew::SrcRow row = {{0, ew::kNoRecord, state == 2 && !clip ? 0u : ew::kNoRecord, state == 2 && clip ? 0u : ew::kNoRecord}, state == 1 ? (uint32_t)ew::SRC_HIT_A : 0u};
    const uint8_t verdict = state == 2 ? ((clip != crossed) ? 32 : 16) : 0;
    dr::Unit U = {arena, arena_len, &row, &verdict, 1, len, st};
    uint64_t bytes = 0;
    uint32_t reads = 0;
    const bool ok = dr::size_unit<ew::HostCtx>(U, bytes, reads);
    if (ok) CHECK(bytes == (uint64_t)len[0] + len[1] && reads == (len[0] ? 1u : 0u) + (len[1] ? 1u : 0u), "bytes %llu reads %u", (unsigned long long)bytes, reads);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: %s cases.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    unsigned n_cases = 0, n_outside = 0, n_prefixes = 0, n_emits = 0;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string kind, rec_hex, want_hex;
        unsigned state = 0;
        f >> kind >> state >> rec_hex >> want_hex;
        if (kind != "E") continue;
        ++n_cases;
        const std::vector<uint8_t> rec = unhex(rec_hex), want = unhex(want_hex);
        const bool inside = want_hex != "-";
        n_outside += inside ? 0 : 1;
        for (unsigned src_shift = 0; src_shift < 4; ++src_shift) {
            // (the arena begins at the record: the offset is 0, the pointer's alignment is the shift)
            Exact arena(rec, rec.size(), src_shift);
            uint32_t len[2] = {77, 77};
            uint8_t st[2] = {9, 9};
            const bool clip = (n_cases + src_shift) % 2 == 1;           // (A through either kind of candidate, in turn)
            const bool ok = decide(arena.p, rec.size(), state, len, st, clip);
            if (state == 2) {                                            // the verdict bit of the candidate the row does not have: refused
                uint32_t l2[2] = {0, 0};
                uint8_t s2[2] = {0, 0};
                CHECK(!decide(arena.p, rec.size(), 2, l2, s2, clip, true), "case %u: a verdict bit without its candidate is taken", n_cases);
            }
            CHECK(ok == inside, "case %u: inside %d, the rules say %d", n_cases, (int)inside, (int)ok);
            if (!ok || !inside) continue;
            // a read that is not set writes its fragment only when something else fired: nothing did here
            const uint32_t want_len = state ? (uint32_t)want.size() : 0u;
            CHECK(len[0] == want_len && len[1] == 0 && st[0] == state && st[1] == 0, "case %u: len %u %u state %u %u", n_cases, len[0], len[1], st[0], st[1]);
            dr::Rec r;
            uint32_t xv = 0;
            CHECK(dr::record_at(arena.p, rec.size(), 0, r) && dr::xv_bytes(r, xv), "case %u: record_at", n_cases);
            const uint32_t emit_len = 4 + r.body_end + (r.size - r.tags_off) - (state ? xv : 0) + (state ? 4 : 0);
            CHECK(emit_len == want.size(), "case %u: %u bytes, bam.py writes %zu", n_cases, emit_len, want.size());
            if (emit_len != want.size()) continue;
            for (unsigned dst_shift = 0; dst_shift < 4; ++dst_shift) {
                Exact dst(want.size(), dst_shift);
                std::memset(dst.p, 0xEE, want.size());
                CHECK(dr::emit_read<ew::HostCtx>(arena.p, rec.size(), 0, (uint8_t)state, dst.p, emit_len), "case %u: emit_read", n_cases);
                CHECK(std::memcmp(dst.p, want.data(), want.size()) == 0, "case %u shift %u -> %u: bytes differ", n_cases, src_shift, dst_shift);
                // a length that is not the record's is refused, and nothing lands behind it
                if (emit_len > 40) {
                    Exact shorter(emit_len - 1, dst_shift);
                    CHECK(!dr::emit_read<ew::HostCtx>(arena.p, rec.size(), 0, (uint8_t)state, shorter.p, emit_len - 1), "case %u: a short destination", n_cases);
                }
                ++n_emits;
            }
            // tag_field against walk_tags over the record's tag area
            rr::Tags t;
            rr::tags_begin(t);
            uint32_t at = r.tags_off, walked = r.tags_off;
            const uint32_t all = rr::walk_tags(r.d, r.size, walked, false, t);
            uint32_t step = rr::TAG_FIELD;
            while (step == rr::TAG_FIELD) { uint32_t next = at; step = rr::tag_field(r.d, r.size, at, next); if (step == rr::TAG_FIELD) at = next; }
            CHECK(step == all, "case %u: tag_field ends with %u, walk_tags with %u", n_cases, step, all);
        }
        if (state != 1) continue;                                      // (the prefixes once per record)
        for (size_t k = 0; k < rec.size(); ++k) {
            for (int fit = 0; fit < 2; ++fit) {
                if (fit && k < 4) continue;
                Exact arena(rec, k, (unsigned)(k & 3));
                if (fit) { const uint32_t size = (uint32_t)(k - 4); for (int i = 0; i < 4; ++i) arena.p[i] = (uint8_t)(size >> (8 * i)); }
                uint32_t len[2] = {0, 0};
                uint8_t st[2] = {0, 0};
                const bool ok = decide(arena.p, k, 1, len, st);
                if (!fit) CHECK(!ok, "case %u: the prefix of %zu bytes is taken", n_cases, k);
                if (ok) {                                              // (a record cut at a field's end, with a block_size to match, is a record)
                    CHECK(len[0] <= k + 4, "case %u prefix %zu: %u bytes", n_cases, k, len[0]);
                    Exact dst(len[0], 0);
                    CHECK(dr::emit_read<ew::HostCtx>(arena.p, k, 0, 1, dst.p, len[0]), "case %u prefix %zu: emit_read", n_cases, k);
                }
                ++n_prefixes;
            }
        }
    }
    std::printf("%u cases, %u outside, %u prefixes, %u emits\n", n_cases, n_outside, n_prefixes, n_emits);
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}

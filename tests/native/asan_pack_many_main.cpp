// AddressSanitizer / UndefinedBehaviorSanitizer harness of the packed-evidence encoder for more than 256 libraries (svt_pack.cpp
// is plain host C++): batches of 300 and 4200 libraries (three per sample) and one whose records alternate between libraries
// 255 and 256 (the last short and the first wide library switch), each through every form of the encoder -- sixteen records at
// a time where the CPU has AVX-512 and record by record, 1 / 3 / 8 workers, the plain and the ranged form -- which must all write the same
// bytes; then the answers that stay: a slot array that is too small, a record naming a library the batch has not, the batch
// without the many_libraries flag.  Built and run by tests/test_packed_many_libraries_native.py with
// g++ -fsanitize=address,undefined; a stand-alone program, nothing is preloaded.  Prints "ok" as its last line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "svt_entry_formats.h"
#include "svt_pack.h"
using namespace svt;

namespace {

struct Batch {
    std::vector<uint64_t> off;
    std::vector<svt_unit> units;
    std::vector<svt_record> recs;
    std::vector<svt_library> libs;
    svt_evidence_batch in{};
};

std::vector<uint32_t> g_hist[3];
svt_library g_tables[3];

void make_tables()
{
    const double mean[3] = {350.37, 420.21, 270.13}, sd[3] = {80.71, 95.02, 40.13};
    const int32_t key_min[3] = {50, 80, 120};
    const uint32_t bins[3] = {600, 700, 300};
    for (int t = 0; t < 3; ++t) {
        g_hist[t].resize(bins[t]);
        for (uint32_t i = 0; i < bins[t]; ++i) {
            const double x = (double)key_min[t] + i - mean[t];
            g_hist[t][i] = 1 + (uint32_t)(1000.0 * std::exp(-0.5 * x * x / (sd[t] * sd[t])));
        }
        g_tables[t] = svt_library{};
        g_tables[t].hist = g_hist[t].data();
        g_tables[t].key_min = key_min[t];
        g_tables[t].n_bins = bins[t];
        g_tables[t].mean = mean[t];
        g_tables[t].sd = sd[t];
    }
}

// library_of(unit, record within the unit, draw) -> library; hint_of(unit) -> svt_unit.libs
template <class LibraryOf, class HintOf>
void fill(Batch& b, uint32_t n_libs, uint64_t n_units, unsigned seed, LibraryOf library_of, HintOf hint_of)
{
    std::mt19937 rng(seed);
    b.off.assign(n_units + 1, 0);
    b.units.assign(n_units, svt_unit{});
    for (uint64_t u = 0; u < n_units; ++u) {
        b.off[u + 1] = b.off[u] + rng() % 41;
        b.units[u].var_length = 300 + (int)(rng() % 2000);
        b.units[u].pos_delta = b.units[u].var_length;
        b.units[u].svtype = rng() % 4;
        b.units[u].libs = hint_of(u);
    }
    b.recs.resize(b.off[n_units]);
    for (uint64_t u = 0; u < n_units; ++u)
        for (uint64_t i = b.off[u]; i < b.off[u + 1]; ++i) {
            svt_record& r = b.recs[i];
            std::memset(&r, 0, sizeof r);
            r.ospan_len = 100 + (int)(rng() % 900);
            r.mapq_a = (i % 5) ? 60 : 37;               // wide entries in front of and behind switches, in every alignment
            r.mapq_b = (rng() % 10) ? 60 : 41;
            r.flags = (rng() % 8) | SVT_REC_HAS_PAIR | (uint32_t)library_of(u, i - b.off[u], rng()) << SVT_REC_LIB_SHIFT;
            r.rs_a = (rng() % 3) ? 0 : 60;
            r.seq_l = (rng() % 20) ? 0 : 40;
            r.clip_r = (rng() % 25) ? 0 : 33;
        }
    b.libs.resize(n_libs);
    for (uint32_t l = 0; l < n_libs; ++l) b.libs[l] = g_tables[l % 3];
    b.in = svt_evidence_batch{};
    b.in.n_units = n_units;
    b.in.rec_offset = b.off.data();
    b.in.units = b.units.data();
    b.in.records = b.recs.data();
    b.in.n_libs = n_libs;
    b.in.libs = b.libs.data();
    b.in.split_weight = 1;
    b.in.disc_weight = 1;
}

void per_sample(Batch& b, uint32_t n_libs, uint64_t n_units, bool hint)
{
    const uint32_t n_samples = (n_libs + 2) / 3;
    auto count = [=](uint64_t u) { return std::min<uint32_t>(3, n_libs - 3 * (uint32_t)(u % n_samples)); };
    fill(b, n_libs, n_units, 1000 + n_libs,
         [=](uint64_t u, uint64_t, uint32_t draw) { return 3 * (uint32_t)(u % n_samples) + draw % count(u); },
         [=](uint64_t u) { return hint ? SVT_UNIT_LIBS(3 * (uint32_t)(u % n_samples), count(u)) : 0u; });
}

void across_the_boundary(Batch& b)
{
    fill(b, 300, 1500, 4242,
         [](uint64_t u, uint64_t k, uint32_t) { return u % 5 ? 255u + (uint32_t)(k % 2) : 254u + 3u * (uint32_t)(k % 2); },
         [](uint64_t) { return SVT_UNIT_LIBS(254, 4); });
}

const PackAlloc kMalloc{[](uint64_t bytes) { return std::malloc(bytes); }, [](void* p) { std::free(p); }};

struct Packed {
    int rc = 0;
    std::vector<uint32_t> off;
    std::vector<unsigned char> units, slots;
    uint32_t common = 0;
    uint64_t handed_units = 0, handed_slots = 0;
    bool operator==(const Packed& o) const { return rc == o.rc && off == o.off && units == o.units && slots == o.slots && common == o.common; }
};

// range_units = 0: the plain call
Packed pack(const Batch& b, uint64_t range_units, uint64_t slots_cap = 0, bool many = true)
{
    Packed p;
    PackSink sink;
    sink.range_units = range_units;
    sink.slots_cap = slots_cap ? slots_cap : b.in.rec_offset[b.in.n_units] + 3 * b.in.n_units + 64;
    sink.ctx = &p;
    sink.ready = [](void* ctx, const PackedArrays* a, uint64_t u0, uint64_t u1, uint64_t s0, uint64_t s1) -> int {
        Packed& q = *static_cast<Packed*>(ctx);
        uint64_t x = 0;                                  // read what was handed over, as the consumer's DMA would
        for (uint64_t i = 16 * s0; i < 16 * s1; ++i) x += static_cast<const unsigned char*>(a->slots)[i];
        for (uint64_t u = u0; u < u1; ++u) x += a->off[3 * u + 3] + (uint64_t)a->units[u].var_length;
        q.handed_units += u1 - u0;
        q.handed_slots += s1 - s0 + (x == 1 ? 0 : 0);
        return 0;
    };
    PackedArrays out;
    p.rc = encode_packed(&b.in, kMalloc, &out, range_units ? &sink : nullptr, many);
    if (p.rc != 0) return p;
    const uint64_t n = b.in.n_units;
    p.off.assign(out.off, out.off + 3 * n + 1);
    p.units.assign(reinterpret_cast<unsigned char*>(out.units), reinterpret_cast<unsigned char*>(out.units + n));
    p.slots.assign(static_cast<unsigned char*>(out.slots), static_cast<unsigned char*>(out.slots) + 16 * out.n_slots);
    p.common = out.common;
    if (p.off[3 * n] != out.n_slots) p.rc = -100;
    if (range_units && (p.handed_units != n || p.handed_slots != out.n_slots)) p.rc = -101;
    kMalloc.put(out.off);
    kMalloc.put(out.units);
    kMalloc.put(out.slots);
    return p;
}

void env(const char* name, const char* value)
{
    if (value) setenv(name, value, 1); else unsetenv(name);
}

// short and wide switches of all pair streams (svt_entry_formats.h: a pair of half-words starts at an even one)
void count_switches(const Batch& b, const Packed& p, uint64_t* n_short, uint64_t* n_wide)
{
    *n_short = *n_wide = 0;
    const uint16_t* half = reinterpret_cast<const uint16_t*>(p.slots.data());
    for (uint64_t u = 0; u < b.in.n_units; ++u)
        for (uint64_t k = 8ull * p.off[3 * u], end = 8ull * p.off[3 * u + 1]; k < end;) {
            const uint16_t h = half[k];
            if (h == kWideSwitch) { ++*n_wide; k += 2; }
            else if (h & 0x8000) k += 2;
            else { if (h && !(h & 7)) ++*n_short; k += 1; }
        }
}

int fail(const char* what, const std::string& which)
{
    std::printf("FAILED %s: %s (last error '%s')\n", which.c_str(), what, g_err.c_str());
    return 1;
}

int all_forms(const Batch& b, const std::string& name)
{
    const Packed want = pack(b, 0);
    if (want.rc != 0) return fail("the plain call", name);
    uint64_t n_short, n_wide;
    count_switches(b, want, &n_short, &n_wide);
    std::printf("%s: %llu units %llu records %zu slots, %llu short and %llu wide switches\n", name.c_str(), (unsigned long long)b.in.n_units,
                (unsigned long long)b.recs.size(), want.slots.size() / 16, (unsigned long long)n_short, (unsigned long long)n_wide);
    if (!n_wide || !n_short) return fail("no wide or no short switch in the pair streams", name);
    for (const char* scalar : {(const char*)nullptr, "1"}) {
        env("SVT_PACK_SCALAR", scalar);
        // (every call builds the libraries' tables again, which is what takes the time here: four combinations, not all nine)
        const struct { const char* threads; uint64_t range; } forms[] = {{"1", 0}, {"8", 0}, {"3", 256}, {"8", 1024}};
        for (const auto& f : forms) {
            env("SVT_PACK_THREADS", f.threads);
            if (!(pack(b, f.range) == want))
                return fail("the forms of the encoder differ", name + (scalar ? " scalar" : "") + " threads " + f.threads + " range " + std::to_string(f.range));
        }
    }
    env("SVT_PACK_SCALAR", nullptr);
    env("SVT_PACK_THREADS", nullptr);
    return 0;
}

}  // namespace

int main()
{
    make_tables();
    std::printf("avx512 %d\n", (int)(__builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("avx512vl") && __builtin_cpu_supports("bmi2")));
    Batch b300, b300_no_hint, b4200, boundary;
    per_sample(b300, 300, 2048, true);
    per_sample(b300_no_hint, 300, 2048, false);
    per_sample(b4200, 4200, 4200, true);
    across_the_boundary(boundary);
    if (all_forms(b300, "300 libraries") || all_forms(b300_no_hint, "300 libraries, no window hint") || all_forms(b4200, "4200 libraries") ||
        all_forms(boundary, "255 / 256 alternating"))
        return 1;

    for (const char* scalar : {(const char*)nullptr, "1"}) {
        env("SVT_PACK_SCALAR", scalar);
        const std::string form = scalar ? "scalar" : "default";
        // a slot array far too small, and one a slot short: the encoder says so and has written nothing past it (the allocation
        // is exactly slots_cap * 16 bytes)
        const uint64_t need = pack(boundary, 0).slots.size() / 16;
        for (uint64_t cap : {(uint64_t)16, need / 2, need - 1})
            if (pack(boundary, 256, cap).rc != SVT_ERR_PACK_OVERFLOW) return fail("a small slot array is not answered with the overflow code", form);
        if (pack(boundary, 256, need).rc != 0) return fail("the exact slot count is refused", form);
        // a record that names a library the batch has not
        for (uint32_t lib : {300u, 4095u, 65535u}) {
            Batch bad = b300;
            bad.in.rec_offset = bad.off.data(); bad.in.units = bad.units.data(); bad.in.records = bad.recs.data(); bad.in.libs = bad.libs.data();
            svt_record& r = bad.recs[bad.off[1700] + (bad.off[1701] > bad.off[1700] ? 0 : 1)];
            r.flags = (r.flags & 0xff) | lib << SVT_REC_LIB_SHIFT;
            for (uint64_t range : {0, 256}) {
                if (pack(bad, range).rc != SVT_ERR_INVALID || g_err.find("lib index") == std::string::npos) return fail("a library index beyond n_libs", form);
            }
        }
        // without the flag the batch stays canonical; 65537 libraries are invalid either way
        if (pack(b300, 0, 0, /*many=*/false).rc != SVT_ERR_UNSUPPORTED) return fail("300 libraries without the flag", form);
        Batch huge = b300;
        huge.in.rec_offset = huge.off.data(); huge.in.units = huge.units.data(); huge.in.records = huge.recs.data(); huge.in.libs = huge.libs.data();
        huge.libs.resize(65537, g_tables[0]);
        huge.in.libs = huge.libs.data();
        huge.in.n_libs = 65537;
        if (pack(huge, 0).rc != SVT_ERR_INVALID) return fail("65537 libraries", form);
    }
    env("SVT_PACK_SCALAR", nullptr);
    pack_trim();
    std::printf("ok\n");
    return 0;
}

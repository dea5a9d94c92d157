// svt_crc32.h -- the CRC-32 of gzip (polynomial 0xEDB88320 reflected, initial value and final xor 0xFFFFFFFF) over the inflated
// bytes of one BGZF member, 0 .. 65 536 of them.
//
// ONE piece of source for both places that run it, as svt_inflate.h is: the host (svt_bgzf_crc32_host, svt_bgzf_inflate_host_verified:
// any C++17 compiler, this is where the split and the combine are proven, fuzzed and sanitised) and the device (svt_crc32_kernel.h,
// hipcc, one wavefront per member).  Written once against a context `X`: X::lane() / X::lanes() / X::sync().  On the host there
// is one lane, which takes the 64 chunks one after the other, and sync() is nothing.
//
// How the lanes share a member.  A CRC is a serial chain over its bytes, but the register is linear in them: with R(s, B) the
// register after the bytes B from the state s,  R(s, A|B) = R(s, A) * x^(8 |B|) mod P  xor  R(0, B).  So the member is cut into
// 64 chunks, every lane runs a table-driven CRC (slicing-by-8, sixteen bytes per load) over its own, and the 64 registers are
// joined by a log-step tree of multiplications mod P.
//
// The cut (plan()).  Loads are 16 bytes wide, so chunks begin and end on 16-byte boundaries of the ADDRESS, and the chunks are laid
// out from the member's END backwards: with `e` the last 16-byte boundary at or in front of the member's end, lane 63 takes
// [e - C, e), lane 62 [e - 2C, e - C) and so on, C = 16 * ceil(whole 16-byte words / 64).  Everything that is ragged lies at the
// FRONT, where a chunk's length does not matter to anybody -- a register is multiplied by x^(8 * the bytes BEHIND its chunk), and
// behind every lane there are whole chunks only, so one power per tree level serves all lanes:
//   * the bytes in front of the first whole chunk (fewer than C + 16: the unaligned lead of up to 15 bytes and the words that
//     do not fill a chunk) are the chunk of the lane in front of the first whole one -- or, when all 64 lanes hold whole chunks,
//     the up to 15 lead bytes go in front of lane 0's chunk.  That lane starts from 0xFFFFFFFF, also when it has no byte at all;
//   * lanes in front of it start from 0 and have no bytes: their registers stay 0 and add nothing, whatever they are multiplied by
//     (members shorter than 64 words: C = 16, and only the last lanes have work);
//   * the up to 15 bytes behind `e` are run through the joined register byte by byte;
//   * a member that crosses no 16-byte boundary at all (fewer than 16 bytes, e in front of its start) is those tail bytes only.
//
// The powers x^(8 * C * 2^s) for the six tree levels and the 64 possible C are a host-built table (Tables.xp, fill_tables());
// the multiplication is a 32-step shift-and-xor in plain integer code: no carry-less multiply is assumed.  No std::, no allocation.
#ifndef SVT_CRC32_H
#define SVT_CRC32_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace crc {

constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kLanes = 64;             // chunks of a member (the device: the lanes of its wavefront)
constexpr uint32_t kLevels = 6;             // log2(kLanes)
constexpr uint32_t kMaxLen = 65536;         // a BGZF member inflates to at most 64 KiB
constexpr uint32_t kMaxWords = kMaxLen / 16 / kLanes;   // 16-byte words of a chunk at most (64)

// built on the host (fill_tables), staged in LDS once per wave on the device
struct Tables {
    uint32_t t[8][256];                     // slicing-by-8
    uint32_t xp[kLevels][kMaxWords + 1];    // xp[s][m] = x^(8 * 16 m * 2^s) mod P
};

struct Scratch { uint32_t r[kLanes]; };     // the lanes' registers on their way through the tree

struct HostCtx {
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
};

// bytes[off, off + len) with the CRC-32 its trailer stores (svt_crc32_kernel.h; `expected` is read only where a status is asked for)
struct Job { uint64_t off; uint32_t len, expected; };

// a * b mod P.  Reflected: bit 31 is x^0, as in the register.
SVT_HD uint32_t mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
#pragma unroll 4
    for (uint32_t i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}

// (host) the byte tables, and the powers by repeated squaring from x^8
inline void fill_tables(Tables& T)
{
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t c = b;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
        T.t[0][b] = c;
    }
    for (uint32_t k = 1; k < 8; ++k)
        for (uint32_t b = 0; b < 256; ++b) T.t[k][b] = (T.t[k - 1][b] >> 8) ^ T.t[0][T.t[k - 1][b] & 0xFF];
    uint32_t x128 = 0x80000000u >> 8;                       // x^8 ...
    for (int k = 0; k < 4; ++k) x128 = mulmod(x128, x128);  // ... squared four times: x^128, one 16-byte word
    T.xp[0][0] = 0x80000000u;                               // x^0
    for (uint32_t m = 1; m <= kMaxWords; ++m) T.xp[0][m] = mulmod(T.xp[0][m - 1], x128);
    for (uint32_t s = 1; s < kLevels; ++s)
        for (uint32_t m = 0; m <= kMaxWords; ++m) T.xp[s][m] = mulmod(T.xp[s - 1][m], T.xp[s - 1][m]);
}

SVT_HD uint32_t step_byte(const Tables& T, uint32_t r, uint8_t b) { return T.t[0][(r ^ b) & 0xFF] ^ (r >> 8); }

SVT_HD uint32_t step_8(const Tables& T, uint32_t r, uint32_t lo, uint32_t hi)
{
    lo ^= r;
    return T.t[7][lo & 0xFF] ^ T.t[6][(lo >> 8) & 0xFF] ^ T.t[5][(lo >> 16) & 0xFF] ^ T.t[4][lo >> 24] ^
           T.t[3][hi & 0xFF] ^ T.t[2][(hi >> 8) & 0xFF] ^ T.t[1][(hi >> 16) & 0xFF] ^ T.t[0][hi >> 24];
}

struct alignas(16) Word16 { uint32_t w[4]; };

// The cut of one member: `words` 16-byte words per whole chunk, the first lane that has a chunk, the bytes of that lane's
// chunk, and the bytes behind the last chunk.  Lane l > first covers [front + (l - first - 1) * 16 words, ... + 16 words) of the
// member, lane `first` covers [0, front).
struct Plan { uint32_t words, first, front, tail; };

SVT_HD Plan plan(const uint8_t* p, uint32_t len)
{
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint32_t end_a = (a + len) & ~15u;                // (address offsets from p - a, which is on a boundary)
    Plan q{0, kLanes - 1, 0, len};
    if (end_a == 0) return q;                               // a + len < 16: no boundary at or in front of its end -- tail bytes only
    const uint32_t body = end_a - a;                        // bytes up to the last boundary
    const uint32_t n16 = body / 16;                         // whole words in them (the lead of body % 16 bytes is in front)
    q.tail = a + len - end_a;
    if (n16 == 0) { q.front = body; return q; }             // (a lead that ends on the boundary, no whole word)
    q.words = (n16 + kLanes - 1) / kLanes;
    const uint32_t whole = n16 / q.words;                   // whole chunks: 1 .. 64
    q.front = body - whole * q.words * 16;
    if (whole < kLanes) q.first = kLanes - 1 - whole;       // a lane of its own for the front (it may hold no byte)
    else { q.first = 0; q.front += q.words * 16; }          // (front < 16 here: the lead goes in front of lane 0's chunk)
    return q;
}

// lane `l`'s register over its chunk
SVT_HD uint32_t lane_register(const uint8_t* p, const Plan& q, const Tables& T, uint32_t l)
{
    if (l < q.first) return 0;
    uint32_t r = 0, at, n;
    if (l == q.first) { r = 0xFFFFFFFFu; at = 0; n = q.front; }
    else { at = q.front + (l - q.first - 1) * q.words * 16; n = q.words * 16; }
    const uint8_t* c = p + at;
    // up to the first boundary byte by byte (only the first lane's chunk begins off one), then sixteen bytes per load
    while (n && (reinterpret_cast<uintptr_t>(c) & 15u)) { r = step_byte(T, r, *c++); --n; }
    for (; n >= 16; n -= 16, c += 16) {
        Word16 v;
        __builtin_memcpy(&v, __builtin_assume_aligned(c, 16), 16);
        r = step_8(T, r, v.w[0], v.w[1]);
        r = step_8(T, r, v.w[2], v.w[3]);
    }
    while (n) { r = step_byte(T, r, *c++); --n; }           // (never taken: a chunk ends on a boundary; kept for a plan that changes)
    return r;
}

// The CRC-32 of p[0, len), len <= kMaxLen; valid on every lane after the call.
template <class X>
SVT_HD uint32_t crc_member(const uint8_t* p, uint32_t len, const Tables& T, Scratch& S)
{
    const Plan q = plan(p, len);
    X::sync();                                              // (nobody still reads the registers of the member before)
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) S.r[l] = lane_register(p, q, T, l);
    X::sync();
    for (uint32_t s = 0; s < kLevels; ++s) {
        const uint32_t power = T.xp[s][q.words];
        for (uint32_t l = X::lane(); l < kLanes; l += X::lanes())
            if ((l & ((2u << s) - 1)) == 0) S.r[l] = mulmod(S.r[l], power) ^ S.r[l + (1u << s)];
        X::sync();
    }
    uint32_t r = S.r[0];
    const uint8_t* t = p + (len - q.tail);
    for (uint32_t i = 0; i < q.tail; ++i) r = step_byte(T, r, t[i]);
    return ~r;
}

}  // namespace crc
}  // namespace svt

#endif  // SVT_CRC32_H

// svt_deflate.h -- the payload of one BGZF member, 0 .. 65 280 bytes, -> its raw-deflate bytes (DESIGN 3.4 is the format).
//
// ONE piece of source for both places that run it, as svt_inflate.h and svt_crc32.h are: the host (svt_bgzf_deflate_host, any
// C++17 compiler: this is where the bytes are proven against the restatement of tests/deflatecases.py and sanitised) and the
// device (svt_deflate_kernel.h, hipcc, one wavefront per member).  Written once against a context `X`: X::lane() / X::lanes() /
// X::sync(), and X::kWidth, the private tables that lie side by side in Scratch (the lanes).  On the host there is one lane,
// which takes the 64 chunks one after the other over one table, and sync() is nothing.
//
// The compressed bytes are a pure function of the payload: the member is cut into 64 chunks of C = ceil(n / 64) bytes, every
// chunk is parsed greedily over a private hash table of 2^kHashBits 16-bit positions that is seeded with the chunk in front,
// and the tokens of all chunks form one fixed-Huffman block (or, where that is no gain, one stored block).  Nothing in the
// result depends on who ran a chunk or when.
//
// How the lanes share a member.  A chunk's tokens are known only after its parse, and where its bits go only after every
// chunk in front of it is parsed.  So a lane parses its chunk twice: once counting bits (Count), and -- behind an exclusive
// prefix sum over the 64 counts in Scratch.start -- once writing them (Writer).  The three header bits are lane 0's first bits
// and the end-of-block code lane 63's last, so the lanes' bit ranges [start[l], start[l + 1]) tile the block.
//
// Bytes that lanes share.  A byte belongs to the lane that holds its first bit; that lane alone stores it.  A lane whose range
// begins inside a byte hands the bits of that byte over in Scratch.head[l] (a plain store of its own entry), the owner leaves
// its own bits of its last byte in Scratch.tail[l], and after one sync() it ORs in the heads of the lanes that begin inside it:
// integer OR of values each written by one lane, so the byte does not depend on arrival order.  A lane with no bits hands
// over 0.  Whole bytes are plain stores.
//
// The tables.  Entry e of lane l is table[e * kWidth + l]: 64 lanes that probe 64 unrelated entries touch dword (e * 32 + l / 2),
// that is bank (l / 2 + 32 (e & 1)) of 64 -- two lanes meet in a bank only where they share a dword.  A match's source may lie
// in the previous lane's chunk: that is payload, which nobody writes, so no sync stands in front of it.
//
// Every read is checked against `n`, every write against `cap`.  No std::, no allocation.
#ifndef SVT_DEFLATE_H
#define SVT_DEFLATE_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace dfl {

constexpr uint32_t kLanes = 64;             // chunks of a member (the device: the lanes of its wavefront)
constexpr uint32_t kMaxPayload = 65280;     // bam.BgzfWriter's payload per member (htslib's block size)
constexpr uint32_t kHashBits = 8;           // t: 64 tables of 256 entries are 32 KiB of LDS per wave
constexpr uint32_t kTable = 1u << kHashBits;
constexpr uint32_t kEmpty = 0xFFFF;         // no position is 65 535: the last one that is hashed is 65 276
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258;
constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8;

// the most a member's deflate bytes take: a stored block (5 + n), or the two bytes of the empty fixed block
SVT_HD uint32_t cdata_bound(uint32_t n) { return n ? n + 5 : 2; }
// the room a member is given before its size is known: header, cdata_bound, trailer
SVT_HD uint32_t slot_bytes(uint32_t n) { return kHeaderBytes + 5 + n + kTrailerBytes; }

// byte i of the 18 header bytes bam.BgzfWriter writes in front of `clen` deflate bytes (BSIZE = clen + 25), and byte i of the
// 8 behind them: the payload's CRC-32 and ISIZE.  Byte by byte, so that the lanes of a copy can each take some.
SVT_HD uint8_t header_byte(uint32_t i, uint32_t clen)
{
    const uint32_t bsize = clen + 25;
    return i == 0 ? 0x1F : i == 1 ? 0x8B : i == 2 ? 8 : i == 3 ? 4 : i == 9 ? 0xFF : i == 10 ? 6 : i == 12 ? 'B' : i == 13 ? 'C' : i == 14 ? 2
           : i == 16 ? (uint8_t)bsize : i == 17 ? (uint8_t)(bsize >> 8) : 0;
}
SVT_HD uint8_t trailer_byte(uint32_t i, uint32_t crc, uint32_t n) { return (uint8_t)((i < 4 ? crc : n) >> (8 * (i & 3))); }

template <uint32_t W>
struct Scratch {
    alignas(4) uint16_t table[kTable * W];  // entry e of table l: table[e * W + l]
    uint32_t start[kLanes + 1];             // counts, then the bit at which lane l's bits begin; [64]: the block's bits
    uint32_t tail[kLanes];                  // bit 31: lane l's last bits begin a byte, (its index << 8) | those bits
    uint8_t head[kLanes];                   // lane l's bits of the byte its range begins in, when it begins inside one
};

struct HostCtx {
    static constexpr uint32_t kWidth = 1;
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
};

SVT_HD uint32_t le32(const uint8_t* p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
SVT_HD uint32_t hash(uint32_t v) { return (v * 2654435761u) >> (32 - kHashBits); }

// the low `n` bits of v, first bit last: a Huffman code goes into the stream first bit first
SVT_HD uint32_t rev(uint32_t v, uint32_t n)
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | (v >> 8);
    return v >> (16 - n);
}

// ---- the fixed Huffman code (RFC 1951 3.2.6): a token as bits, lowest first, and how many -------------------------------------
SVT_HD uint32_t literal_bits(uint32_t b, uint32_t& n)
{
    if (b < 144) { n = 8; return rev(0x30 + b, 8); }
    n = 9;
    return rev(0x190 + (b - 144), 9);
}

// match (len 3 .. 258, dist 1 .. 32 768): length code, its extra bits, distance code, its extra bits -- 31 bits at most
SVT_HD uint32_t match_bits(uint32_t len, uint32_t dist, uint32_t& n)
{
    uint32_t sym, eb = 0, ev = 0;
    const uint32_t l = len - 3;
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + l;
    else {
        eb = (31 - (uint32_t)__builtin_clz(l)) - 2;
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        ev = l & ((1u << eb) - 1);
    }
    uint32_t v;
    if (sym < 280) { v = rev(sym - 256, 7); n = 7; }
    else { v = rev(0xC0 + (sym - 280), 8); n = 8; }
    v |= ev << n;
    n += eb;
    uint32_t dsym, deb = 0, dev = 0;
    const uint32_t d = dist - 1;
    if (d < 4) dsym = d;
    else {
        const uint32_t hb = 31 - (uint32_t)__builtin_clz(d);
        deb = hb - 1;
        dsym = 2 * hb + ((d >> deb) & 1);
        dev = d & ((1u << deb) - 1);
    }
    v |= rev(dsym, 5) << n;
    n += 5;
    v |= dev << n;
    n += deb;
    return v;
}

// ---- the two things a parse feeds ------------------------------------------------------------------------------------------
struct Count {
    uint32_t bits;
    SVT_HD void put(uint32_t, uint32_t n) { bits += n; }
};

// bits from `start` on into out[0, cap): whole bytes as they fill, the byte the range begins inside (if any) into `head`
struct Writer {
    uint8_t* out;
    uint32_t cap, at, nbits;
    uint64_t acc;
    bool shared;            // the byte being filled began in front of this range: it is somebody else's
    uint8_t head;
    SVT_HD void begin(uint8_t* out_, uint32_t cap_, uint32_t start)
    {
        out = out_; cap = cap_; at = start >> 3; nbits = start & 7; acc = 0; shared = nbits != 0; head = 0;
    }
    SVT_HD void put(uint32_t v, uint32_t n)
    {
        acc |= (uint64_t)v << nbits;
        nbits += n;
        while (nbits >= 8) {
            if (shared) { head = (uint8_t)acc; shared = false; }
            else if (at < cap) out[at] = (uint8_t)acc;
            ++at;
            acc >>= 8;
            nbits -= 8;
        }
    }
    // the bits left over: true when they begin a byte (this range owns it: `tail` at out[at]), false when they went to `head`
    SVT_HD bool end(uint8_t& tail)
    {
        tail = (uint8_t)acc;
        if (nbits && shared) { head = (uint8_t)acc; return false; }
        return nbits != 0;
    }
};

// Chunk `l` of p[0, n) parsed greedily over the table at `col` (entries W apart), the tokens put into `sink`.
template <uint32_t W, class Sink>
SVT_HD void parse_chunk(const uint8_t* p, uint32_t n, uint32_t C, uint32_t l, uint16_t* col, Sink& sink)
{
    const uint32_t a = l * C;
    if (a >= n) return;                                     // a chunk behind the payload's end
    const uint32_t b = a + C < n ? a + C : n;
    for (uint32_t e = 0; e < kTable; ++e) col[e * W] = (uint16_t)kEmpty;
    for (uint32_t i = a > C ? a - C : 0; i < a; ++i)       // the seed: the chunk in front
        if (i + 4 <= n) col[hash(le32(p + i)) * W] = (uint16_t)i;
    uint32_t i = a;
    while (i < b) {
        uint32_t m = 0, j = 0, h = 0;
        const bool hashed = i + 4 <= n;
        if (hashed) {
            const uint32_t v = le32(p + i);
            h = hash(v);
            j = col[h * W];
            const uint32_t lim = b - i < kMaxMatch ? b - i : kMaxMatch;
            if (j != kEmpty && lim >= kMinMatch && le32(p + j) == v) {         // (j < i: j + 4 <= n as well)
                m = kMinMatch;
                while (m < lim && p[j + m] == p[i + m]) ++m;
            }
        }
        uint32_t nb;
        if (m) {
            const uint32_t v = match_bits(m, i - j, nb);
            sink.put(v, nb);
            for (uint32_t k = i; k < i + m; ++k)
                if (k + 4 <= n) col[hash(le32(p + k)) * W] = (uint16_t)k;
            i += m;
        } else {
            const uint32_t v = literal_bits(p[i], nb);
            sink.put(v, nb);
            if (hashed) col[h * W] = (uint16_t)i;
            ++i;
        }
    }
}

// p[0, n), n <= kMaxPayload, deflated into out[0, cap), cap >= cdata_bound(n).  Returns the bytes written, the same on every
// lane; 0: refused (n or cap out of range), nothing is written.
template <class X>
SVT_HD uint32_t deflate_member(const uint8_t* p, uint32_t n, uint8_t* out, uint32_t cap, Scratch<X::kWidth>& S)
{
    constexpr uint32_t W = X::kWidth;
    if (n > kMaxPayload || cap < cdata_bound(n)) return 0;
    const uint32_t C = (n + kLanes - 1) / kLanes;
    X::sync();                                              // (nobody still reads start / head of the member before)
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
        Count c{(l == 0 ? 3u : 0u) + (l == kLanes - 1 ? 7u : 0u)};
        parse_chunk<W>(p, n, C, l, S.table + l % W, c);
        S.start[l] = c.bits;
        S.head[l] = 0;
    }
    X::sync();
    if (X::lane() == 0) {                                   // the exclusive prefix sum: 64 steps of one lane, in lane order
        uint32_t at = 0;
        for (uint32_t l = 0; l < kLanes; ++l) { const uint32_t c = S.start[l]; S.start[l] = at; at += c; }
        S.start[kLanes] = at;
    }
    X::sync();
    const uint32_t F = (S.start[kLanes] + 7) / 8;
    if (n > 0 && F >= 5 + n) {                              // no gain: one stored block
        for (uint32_t i = X::lane(); i < 5 + n; i += X::lanes())
            out[i] = i == 0 ? 1 : i == 1 ? (uint8_t)n : i == 2 ? (uint8_t)(n >> 8) : i == 3 ? (uint8_t)~n : i == 4 ? (uint8_t)(~n >> 8) : p[i - 5];
        return 5 + n;
    }
    // (F < 5 + n <= cap, or n == 0 and F == 2 <= cap: every byte of the block has its place)
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
        Writer w;
        w.begin(out, cap, S.start[l]);
        if (l == 0) w.put(3, 3);                            // BFINAL = 1, BTYPE = 01
        parse_chunk<W>(p, n, C, l, S.table + l % W, w);
        if (l == kLanes - 1) w.put(0, 7);                   // end of block
        uint8_t tail;
        const bool owns = w.end(tail);
        S.head[l] = w.head;
        S.tail[l] = owns ? (0x80000000u | (w.at << 8) | tail) : 0;
    }
    X::sync();
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
        const uint32_t t = S.tail[l];
        if (!(t & 0x80000000u)) continue;
        const uint32_t at = (t >> 8) & 0x1FFFFu;            // the byte this lane's last bits begin: its to store
        uint32_t v = t & 0xFF;
        for (uint32_t j = l + 1; j < kLanes && S.start[j] < 8 * (at + 1); ++j) v |= S.head[j];
        if (at < cap) out[at] = (uint8_t)v;
    }
    return F;
}

}  // namespace dfl
}  // namespace svt

#endif  // SVT_DEFLATE_H

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
// The dynamic mode (deflate_member<X, kDynamic>; DESIGN 3.4, "the dynamic block").  The same tokens under a code made for the
// member: a histogram of the tokens of all chunks (every lane adds its chunk's symbols into Scratch.code.freq through
// X::add: sums of integers, the same whatever the order), code lengths from the frequencies alone (code_lengths: the symbols
// ranked across the lanes, the Huffman depths, their repair and the header by lane 0), a second counting parse under that
// code, and the choice: the dynamic block is written only where it is strictly shorter than what the fixed mode writes,
// which is written byte for byte otherwise.  So a chunk is parsed three times; no token is kept anywhere.  The header's bits
// are lane 0's first bits.
//
// Every read is checked against `n`, every write against `cap`.  No std::, no allocation.
#ifndef SVT_DEFLATE_H
#define SVT_DEFLATE_H

#include <stdint.h>

#include "svt_geometry_math.h"

// (a loop that is kept a loop: unrolled over the constant sizes of the small alphabets, the ranking below holds every `t < s`
// in a register pair of its own)
#if defined(__clang__)
#define SVT_DFL_KEEP_LOOP _Pragma("clang loop unroll(disable)")
#else
#define SVT_DFL_KEEP_LOOP _Pragma("GCC unroll 1")
#endif

namespace svt {
namespace dfl {

constexpr uint32_t kLanes = 64;             // chunks of a member (the device: the lanes of its wavefront)
constexpr uint32_t kMaxPayload = 65280;     // bam.BgzfWriter's payload per member (htslib's block size)
constexpr uint32_t kHashBits = 8;           // t: 64 tables of 256 entries are 32 KiB of LDS per wave
constexpr uint32_t kTable = 1u << kHashBits;
constexpr uint32_t kEmpty = 0xFFFF;         // no position is 65 535: the last one that is hashed is 65 276
constexpr uint32_t kMinMatch = 4, kMaxMatch = 258;
constexpr uint32_t kHeaderBytes = 18, kTrailerBytes = 8;
constexpr uint32_t kFixed = 0, kDynamic = 1;                    // the block a member may be written as (deflate_member's mode)
constexpr uint32_t kLitSyms = 286, kDistSyms = 30, kClSyms = 19; // the three alphabets of a dynamic block, side by side:
constexpr uint32_t kDistAt = kLitSyms, kClAt = kLitSyms + kDistSyms, kSyms = kClAt + kClSyms;
constexpr uint32_t kEob = 256;

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

// what one code's construction works in (code_lengths)
struct Build {
    uint32_t w[kLitSyms];                   // weights in rising order -> parents -> depths (Moffat and Katajainen, in place)
    uint32_t cnt[16];                       // symbols per code length
    uint32_t next[16];                      // the next code of each length (canonical_codes)
    uint16_t order[kLitSyms];               // the used symbols by (frequency, symbol), rising
};

// the dynamic mode's part of Scratch: literal/length symbols at 0, distance symbols at kDistAt, code-length symbols at kClAt
struct Code {
    uint32_t freq[kSyms];
    uint32_t dstart[kLanes];                // lane l's bits under the dynamic code
    uint32_t hlit, hdist, hclen, header_bits;
    uint32_t dynamic;                       // the choice: 1: the dynamic block is written
    Build build;
    uint16_t code[kSyms];                   // first bit lowest, as the stream takes it
    uint8_t len[kSyms];
};

template <uint32_t W, uint32_t M = kFixed>
struct Scratch {
    alignas(4) uint16_t table[kTable * W];  // entry e of table l: table[e * W + l]
    uint32_t start[kLanes + 1];             // counts, then the bit at which lane l's bits begin; [64]: the block's bits
    uint32_t tail[kLanes];                  // bit 31: lane l's last bits begin a byte, (its index << 8) | those bits
    uint8_t head[kLanes];                   // lane l's bits of the byte its range begins in, when it begins inside one
};
template <uint32_t W>
struct Scratch<W, kDynamic> : Scratch<W, kFixed> {
    Code code;
};

struct HostCtx {
    static constexpr uint32_t kWidth = 1;
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
    static SVT_HD void add(uint32_t* counter) { ++*counter; }
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

// ---- a match as symbols (RFC 1951 3.2.5): the symbol, how many extra bits and their value -----------------------------------------
SVT_HD uint32_t length_symbol(uint32_t len, uint32_t& eb, uint32_t& ev)
{
    const uint32_t l = len - 3;
    eb = 0; ev = 0;
    if (len == 258) return 285;
    if (l < 8) return 257 + l;
    eb = (31 - (uint32_t)__builtin_clz(l)) - 2;
    ev = l & ((1u << eb) - 1);
    return 261 + 4 * eb + ((l >> eb) & 3);
}
SVT_HD uint32_t distance_symbol(uint32_t dist, uint32_t& deb, uint32_t& dev)
{
    const uint32_t d = dist - 1;
    deb = 0; dev = 0;
    if (d < 4) return d;
    const uint32_t hb = 31 - (uint32_t)__builtin_clz(d);
    deb = hb - 1;
    dev = d & ((1u << deb) - 1);
    return 2 * hb + ((d >> deb) & 1);
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
    uint32_t eb, ev, deb, dev;
    const uint32_t sym = length_symbol(len, eb, ev), dsym = distance_symbol(dist, deb, dev);
    uint32_t v;
    if (sym < 280) { v = rev(sym - 256, 7); n = 7; }
    else { v = rev(0xC0 + (sym - 280), 8); n = 8; }
    v |= ev << n;
    n += eb;
    v |= rev(dsym, 5) << n;
    n += 5;
    v |= dev << n;
    n += deb;
    return v;
}

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

// ---- the things a parse feeds: a chunk's tokens counted or written, under the fixed code or the member's own -------------------
struct Count {
    uint32_t bits;
    SVT_HD void literal(uint32_t b) { uint32_t n; (void)literal_bits(b, n); bits += n; }
    SVT_HD void match(uint32_t len, uint32_t dist) { uint32_t n; (void)match_bits(len, dist, n); bits += n; }
};

struct FixedWrite {
    Writer& w;
    SVT_HD void literal(uint32_t b) { uint32_t n; const uint32_t v = literal_bits(b, n); w.put(v, n); }
    SVT_HD void match(uint32_t len, uint32_t dist) { uint32_t n; const uint32_t v = match_bits(len, dist, n); w.put(v, n); }
};

// the fixed count, and the tokens' symbols into the member's histogram
template <class X>
struct CountAndTally {
    uint32_t bits;
    uint32_t* freq;
    SVT_HD void literal(uint32_t b) { uint32_t n; (void)literal_bits(b, n); bits += n; X::add(freq + b); }
    SVT_HD void match(uint32_t len, uint32_t dist)
    {
        uint32_t n, eb, ev;
        (void)match_bits(len, dist, n);
        bits += n;
        X::add(freq + length_symbol(len, eb, ev));
        X::add(freq + kDistAt + distance_symbol(dist, eb, ev));
    }
};

struct DynamicCount {
    uint32_t bits;
    const uint8_t* len;
    SVT_HD void literal(uint32_t b) { bits += len[b]; }
    SVT_HD void match(uint32_t length, uint32_t dist)
    {
        uint32_t eb, ev, deb, dev;
        const uint32_t sym = length_symbol(length, eb, ev), dsym = distance_symbol(dist, deb, dev);
        bits += len[sym] + eb + len[kDistAt + dsym] + deb;
    }
};

struct DynamicWrite {
    Writer& w;
    const uint16_t* code;
    const uint8_t* len;
    SVT_HD void literal(uint32_t b) { w.put(code[b], len[b]); }
    SVT_HD void match(uint32_t length, uint32_t dist)
    {
        uint32_t eb, ev, deb, dev;
        const uint32_t sym = length_symbol(length, eb, ev), dsym = distance_symbol(dist, deb, dev);
        w.put(code[sym] | (ev << len[sym]), len[sym] + eb);                                      // 15 + 5 bits at most
        w.put(code[kDistAt + dsym] | (dev << len[kDistAt + dsym]), len[kDistAt + dsym] + deb);   // 15 + 13
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
        if (m) {
            sink.match(m, i - j);
            for (uint32_t k = i; k < i + m; ++k)
                if (k + 4 <= n) col[hash(le32(p + k)) * W] = (uint16_t)k;
            i += m;
        } else {
            sink.literal(p[i]);
            if (hashed) col[h * W] = (uint16_t)i;
            ++i;
        }
    }
}

// ---- the member's own code ("the dynamic block") ------------------------------------------------------------------
// Code lengths of at most `limit` bits (limit <= 15) for freq[0, nsym), nsym <= kLitSyms, the frequencies' sum below 2^32 and no
// more than 2^limit of them above zero -- a function of the frequencies alone, in integers:
//   the used symbols (frequency > 0) in rising order of (frequency, symbol);  none: no code;  one: one bit;  else
//   Huffman's tree over them: the two smallest weights are joined until one is left, and among equal weights a leaf goes before
//     a joined node, leaves in their order, nodes in the order they were made -- this gives the depths as a multiset;
//   depths above `limit` become `limit`, and for every unit by which sum 2^(limit - depth) then exceeds 2^limit, one symbol of
//     the greatest depth below `limit` that has one goes one level down and takes one symbol of depth `limit` up beside it
//     (counts only: cnt[d] -= 1, cnt[d + 1] += 2, cnt[limit] -= 1; the sum falls by exactly one: zlib's repair);
//   the lengths are handed out in the symbols' order, the longest first.
// Where the tree fits the limit this is Huffman's optimum.  All lanes call it; freq is complete and B free behind the sync() it
// begins with, len is complete behind the one it ends with.  The ranking is the lanes' (every lane ranks its symbols against
// all others: reads of one address by all lanes), the rest -- a chain of dependent steps over at most 286 entries -- lane 0's.
template <class X>
SVT_HD void code_lengths(const uint32_t* freq, uint32_t nsym, uint32_t limit, uint8_t* len, Build& B)
{
    X::sync();
    for (uint32_t s = X::lane(); s < nsym; s += X::lanes()) {
        const uint32_t f = freq[s];
        len[s] = 0;
        if (!f) continue;
        uint32_t rank = 0;
        SVT_DFL_KEEP_LOOP
        for (uint32_t t = 0; t < nsym; ++t) {
            const uint32_t g = freq[t];
            rank += g && (g < f || (g == f && t < s));
        }
        B.order[rank] = (uint16_t)s;                        // (ranks are a permutation of 0 .. used - 1: below nsym)
    }
    X::sync();
    if (X::lane() == 0) {
        uint32_t m = 0;
        SVT_DFL_KEEP_LOOP
        for (uint32_t t = 0; t < nsym; ++t) m += freq[t] != 0;
        uint32_t* A = B.w;
        for (uint32_t i = 0; i < m; ++i) A[i] = freq[B.order[i]];
        if (m == 1) len[B.order[0]] = 1;
        if (m >= 2) {
            // first pass, left to right: the joined nodes' weights, a used-up node's place taken by its parent's index
            A[0] += A[1];
            uint32_t root = 0, leaf = 2;
            for (uint32_t next = 1; next + 1 < m; ++next) {
                if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
                else A[next] = A[leaf++];
                if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
                else A[next] += A[leaf++];
            }
            // second pass, right to left: the nodes' depths
            A[m - 2] = 0;
            for (uint32_t next = m - 2; next-- > 0;) A[next] = A[A[next]] + 1;
            // third pass, right to left: the leaves' depths, falling
            uint32_t avbl = 1, used = 0, depth = 0;
            int32_t r = (int32_t)m - 2, next = (int32_t)m - 1;
            while (avbl > 0) {
                while (r >= 0 && A[r] == depth) { ++used; --r; }
                while (avbl > used && next >= 0) { A[next--] = depth; --avbl; }
                if (avbl > used) break;                     // (never: the leaves are out exactly when no place is left)
                avbl = 2 * used; ++depth; used = 0;
            }
            for (uint32_t d = 0; d < 16; ++d) B.cnt[d] = 0;
            uint32_t kraft = 0;
            for (uint32_t i = 0; i < m; ++i) {
                const uint32_t d = A[i] < limit ? A[i] : limit;
                ++B.cnt[d];
                kraft += 1u << (limit - d);
            }
            for (uint32_t over = kraft - (1u << limit); over > 0; --over) {
                uint32_t d = limit - 1;
                while (d > 1 && B.cnt[d] == 0) --d;
                if (B.cnt[d] == 0 || B.cnt[limit] == 0) break;  // (never, with at most 2^limit symbols)
                --B.cnt[d]; B.cnt[d + 1] += 2; --B.cnt[limit];
            }
            uint32_t i = 0;
            for (uint32_t d = limit; d >= 1; --d)
                for (uint32_t c = B.cnt[d]; c > 0 && i < m; --c) len[B.order[i++]] = (uint8_t)d;
        }
    }
    X::sync();
}

// the canonical codes of len[0, nsym) (RFC 1951 3.2.2), each turned round for the stream; one lane's
SVT_HD void canonical_codes(const uint8_t* len, uint32_t nsym, uint16_t* code, Build& B)
{
    uint32_t* count = B.cnt;
    uint32_t* next = B.next;
    for (uint32_t d = 0; d < 16; ++d) count[d] = 0;
    SVT_DFL_KEEP_LOOP
    for (uint32_t s = 0; s < nsym; ++s) ++count[len[s] & 15];
    count[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (uint32_t d = 1; d < 16; ++d) { c = (c + count[d - 1]) << 1; next[d] = c; }
    SVT_DFL_KEEP_LOOP
    for (uint32_t s = 0; s < nsym; ++s) {
        const uint32_t d = len[s] & 15;
        code[s] = d ? (uint16_t)rev(next[d]++, d) : 0;
    }
}

// The code lengths len[0, n) as the run-length operations of the header, each to sink.op(symbol, extra): a run of zeros as 18s
// of up to 138 while 11 or more are left, then one 17 for 3 .. 10, then single zeros; a run of another length as that length,
// then 16s of up to 6 while 3 or more are left, then the length itself.  (Literal/length and distance lengths are run through
// separately: no run crosses from one into the other.)
template <class Sink>
SVT_HD void run_length_ops(const uint8_t* len, uint32_t n, Sink& sink)
{
    uint32_t i = 0;
    while (i < n) {
        const uint32_t v = len[i];
        uint32_t run = 1;
        while (i + run < n && len[i + run] == v) ++run;
        uint32_t left = run;
        if (v == 0) {
            while (left >= 11) { const uint32_t take = left < 138 ? left : 138; sink.op(18, take - 11); left -= take; }
            if (left >= 3) { sink.op(17, left - 3); left = 0; }
        } else {
            sink.op(v, 0);
            --left;
            while (left >= 3) { const uint32_t take = left < 6 ? left : 6; sink.op(16, take - 3); left -= take; }
        }
        for (; left > 0; --left) sink.op(v, 0);
        i += run;
    }
}
SVT_HD uint32_t op_extra_bits(uint32_t sym) { return sym < 16 ? 0 : sym == 16 ? 2 : sym == 17 ? 3 : 7; }
struct OpTally {
    uint32_t* freq;
    SVT_HD void op(uint32_t sym, uint32_t) { ++freq[sym]; }
};
struct OpWrite {
    Writer& w;
    const uint16_t* code;
    const uint8_t* len;
    SVT_HD void op(uint32_t sym, uint32_t extra) { w.put(code[sym] | (extra << len[sym]), len[sym] + op_extra_bits(sym)); }
};
// the order in which the header names the code-length code's lengths
SVT_HD uint32_t cl_order(uint32_t i)
{
    static constexpr uint8_t order[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// The histogram of a member's tokens (K.freq, literal/length and distance symbols, the end-of-block not yet in it) -> the three
// sets of lengths, their codes, HLIT / HDIST / HCLEN and the header's bits.  All lanes call it.
template <class X>
SVT_HD void build_code(Code& K)
{
    if (X::lane() == 0) ++K.freq[kEob];
    code_lengths<X>(K.freq, kLitSyms, 15, K.len, K.build);
    code_lengths<X>(K.freq + kDistAt, kDistSyms, 15, K.len + kDistAt, K.build);
    for (uint32_t s = X::lane(); s < kClSyms; s += X::lanes()) K.freq[kClAt + s] = 0;
    X::sync();
    if (X::lane() == 0) {
        uint32_t hlit = kLitSyms, hdist = kDistSyms;
        while (hlit > 257 && K.len[hlit - 1] == 0) --hlit;
        while (hdist > 1 && K.len[kDistAt + hdist - 1] == 0) --hdist;
        if (hdist == 1 && K.len[kDistAt] == 0) K.len[kDistAt] = 1;    // no match in the member: one distance code of one bit
        K.hlit = hlit;
        K.hdist = hdist;
        OpTally tally{K.freq + kClAt};
        run_length_ops(K.len, hlit, tally);
        run_length_ops(K.len + kDistAt, hdist, tally);
    }
    code_lengths<X>(K.freq + kClAt, kClSyms, 7, K.len + kClAt, K.build);
    if (X::lane() == 0) {
        canonical_codes(K.len, kLitSyms, K.code, K.build);
        canonical_codes(K.len + kDistAt, kDistSyms, K.code + kDistAt, K.build);
        canonical_codes(K.len + kClAt, kClSyms, K.code + kClAt, K.build);
        uint32_t hclen = kClSyms;
        while (hclen > 4 && K.len[kClAt + cl_order(hclen - 1)] == 0) --hclen;
        K.hclen = hclen;
        uint32_t bits = 3 + 5 + 5 + 4 + 3 * hclen;
        SVT_DFL_KEEP_LOOP
        for (uint32_t s = 0; s < kClSyms; ++s) bits += K.freq[kClAt + s] * (K.len[kClAt + s] + op_extra_bits(s));
        K.header_bits = bits;
    }
    X::sync();
}

// the header of the dynamic block: BFINAL = 1, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code's lengths, the operations
SVT_HD void write_dynamic_header(const Code& K, Writer& w)
{
    w.put(5, 3);
    w.put(K.hlit - 257, 5);
    w.put(K.hdist - 1, 5);
    w.put(K.hclen - 4, 4);
    SVT_DFL_KEEP_LOOP
    for (uint32_t i = 0; i < K.hclen; ++i) w.put(K.len[kClAt + cl_order(i)], 3);
    OpWrite ops{w, K.code + kClAt, K.len + kClAt};
    run_length_ops(K.len, K.hlit, ops);
    run_length_ops(K.len + kDistAt, K.hdist, ops);
}

// p[0, n), n <= kMaxPayload, deflated into out[0, cap), cap >= cdata_bound(n).  Returns the bytes written, the same on every
// lane; 0: refused (n or cap out of range), nothing is written.  M = kDynamic: the dynamic block where it is strictly shorter
// than what M = kFixed writes, those bytes otherwise.
template <class X, uint32_t M = kFixed>
SVT_HD uint32_t deflate_member(const uint8_t* p, uint32_t n, uint8_t* out, uint32_t cap, Scratch<X::kWidth, M>& S)
{
    constexpr uint32_t W = X::kWidth;
    if (n > kMaxPayload || cap < cdata_bound(n)) return 0;
    const uint32_t C = (n + kLanes - 1) / kLanes;
    X::sync();                                              // (nobody still reads start / head of the member before)
    if constexpr (M == kDynamic) {
        for (uint32_t s = X::lane(); s < kClAt; s += X::lanes()) S.code.freq[s] = 0;
        X::sync();
    }
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
        const uint32_t ends = (l == 0 ? 3u : 0u) + (l == kLanes - 1 ? 7u : 0u);
        if constexpr (M == kDynamic) {
            CountAndTally<X> c{ends, S.code.freq};
            parse_chunk<W>(p, n, C, l, S.table + l % W, c);
            S.start[l] = c.bits;
        } else {
            Count c{ends};
            parse_chunk<W>(p, n, C, l, S.table + l % W, c);
            S.start[l] = c.bits;
        }
        S.head[l] = 0;
    }
    if constexpr (M == kDynamic) {
        build_code<X>(S.code);                              // (begins with a sync())
        for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
            DynamicCount c{(l == 0 ? S.code.header_bits : 0u) + (l == kLanes - 1 ? S.code.len[kEob] : 0u), S.code.len};
            parse_chunk<W>(p, n, C, l, S.table + l % W, c);
            S.code.dstart[l] = c.bits;
        }
    }
    X::sync();
    if (X::lane() == 0) {                                   // the exclusive prefix sum: 64 steps of one lane, in lane order
        if constexpr (M == kDynamic) {                      // ... over the counts of the block that is going to be written
            uint32_t fixed = 0, dynamic = 0;
            SVT_DFL_KEEP_LOOP
            for (uint32_t l = 0; l < kLanes; ++l) { fixed += S.start[l]; dynamic += S.code.dstart[l]; }
            const uint32_t F = (fixed + 7) / 8, D = (dynamic + 7) / 8;
            S.code.dynamic = D < (n > 0 && F >= 5 + n ? 5 + n : F);
            if (S.code.dynamic)
                SVT_DFL_KEEP_LOOP
                for (uint32_t l = 0; l < kLanes; ++l) S.start[l] = S.code.dstart[l];
        }
        uint32_t at = 0;
        for (uint32_t l = 0; l < kLanes; ++l) { const uint32_t c = S.start[l]; S.start[l] = at; at += c; }
        S.start[kLanes] = at;
    }
    X::sync();
    const uint32_t F = (S.start[kLanes] + 7) / 8;           // (the dynamic block's bytes where that was chosen: below 5 + n)
    if (n > 0 && F >= 5 + n) {                              // no gain: one stored block
        for (uint32_t i = X::lane(); i < 5 + n; i += X::lanes())
            out[i] = i == 0 ? 1 : i == 1 ? (uint8_t)n : i == 2 ? (uint8_t)(n >> 8) : i == 3 ? (uint8_t)~n : i == 4 ? (uint8_t)(~n >> 8) : p[i - 5];
        return 5 + n;
    }
    // (F < 5 + n <= cap, or n == 0 and F == 2 <= cap: every byte of the block has its place)
    bool dynamic = false;
    if constexpr (M == kDynamic) dynamic = S.code.dynamic != 0;
    for (uint32_t l = X::lane(); l < kLanes; l += X::lanes()) {
        Writer w;
        w.begin(out, cap, S.start[l]);
        if constexpr (M == kDynamic) {
            if (dynamic) {
                if (l == 0) write_dynamic_header(S.code, w);
                DynamicWrite sink{w, S.code.code, S.code.len};
                parse_chunk<W>(p, n, C, l, S.table + l % W, sink);
                if (l == kLanes - 1) w.put(S.code.code[kEob], S.code.len[kEob]);
            }
        }
        if (!dynamic) {
            if (l == 0) w.put(3, 3);                        // BFINAL = 1, BTYPE = 01
            FixedWrite sink{w};
            parse_chunk<W>(p, n, C, l, S.table + l % W, sink);
            if (l == kLanes - 1) w.put(0, 7);               // end of block
        }
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

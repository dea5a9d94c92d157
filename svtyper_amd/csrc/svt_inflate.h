// svt_inflate.h -- the raw-deflate payload of one BGZF member -> exactly ISIZE bytes, or a status.
//
// ONE piece of source for both places that run it, as svt_evidence_walk.h is: the host (svt_bgzf_inflate_host and the open-range
// arena of svt_reads_arena.h / svt_reads_walk.h, any C++17 compiler: this is where the decoder is proven, fuzzed and sanitised) and the device
// (svt_inflate_kernel.h, hipcc, one wavefront per member).  Written once against a context `X`: X::lane() / X::lanes() /
// X::sync().  On the host there is one lane and sync() is nothing.
//
// The verdict is the host reader's (Bgzf::inflate_block) and zlib's: success means the stream ends with its final block having
// produced exactly ISIZE bytes.  Bytes behind the final block are not looked at.  The CRC32 of the trailer is not this decoder's
// business: it is checked behind it, under verify, by svt_crc32.h (INF_CRC: svt_bgzf_inflate_*_verified, svt_bam_set_verify).  Every input read is
// checked against `clen`, every output write against `isize`, every distance against the bytes produced so far; code-length sets
// are checked for over- and under-subscription as zlib's inflate_table does (an incomplete set only with a single code of one
// bit; no codes at all only for distances); every loop consumes input bits or ends.  No std::, no allocation.
//
// How the lanes share the work.  A deflate stream is one serial chain of bits, so lane 0 owns the bit buffer: it reads the block
// header and the code lengths, and decodes symbols kBatch at a time into Scratch (a literal, or length + distance, each with its
// output position).  Everything else is every lane's: the window of compressed bytes lane 0 reads from (Scratch.in, refilled per
// batch), the fast decode tables, the stored-block copy and the emission of a batch -- first all its literals as byte stores,
// then its matches in order, each copied by the whole wave with the overlap rule (dist < len repeats the last dist bytes).
// A match reads output bytes an earlier store of this wave has written: X::sync() stands between them (svt_inflate_kernel.h says
// what it is on the device).  Lane 0 marks the matches whose source overlaps a match of the same batch that has no sync behind
// it yet; only those pay one.
#ifndef SVT_INFLATE_H
#define SVT_INFLATE_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace inf {

enum : uint32_t {
    INF_OK = 0,
    INF_INPUT = 1,           // the payload ends inside the stream
    INF_BTYPE = 2,           // block type 3
    INF_STORED = 3,          // stored block: LEN / NLEN do not agree
    INF_LENGTHS = 4,         // code lengths: too many symbols, bad repeat, over- / under-subscribed set, no end-of-block code
    INF_SYMBOL = 5,          // bits that are no code of the set / literal-length symbol 286, 287
    INF_DISTANCE = 6,        // distance symbol 30, 31 / distance beyond the bytes produced so far
    INF_OUTPUT = 7,          // more than ISIZE bytes
    INF_SHORT = 8,           // the stream ends with fewer than ISIZE bytes
    INF_MEMBER = 9,          // not a BGZF member, or it does not fit the bytes / the place it was given (decided by the caller)
    INF_CRC = 10,            // (verify only) the member inflated to ISIZE bytes whose CRC-32 is not the trailer's (svt_crc32.h)
    INF_N_STATUS = 11
};

constexpr uint32_t kFastBits = 10;          // literal/length codes up to this length: one look-up
constexpr uint32_t kDistFastBits = 8;
constexpr uint32_t kBatch = 128;            // symbols lane 0 decodes before the lanes emit them
constexpr uint32_t kInWindow = 1024;        // compressed bytes staged per batch (a symbol takes 48 bits at most, a dynamic header 562 bytes)
constexpr uint32_t kMaxIsize = 65536;       // a BGZF member inflates to at most 64 KiB

struct Scratch {
    uint16_t lit_fast[1u << kFastBits];     // (symbol << 4 | code length) under every index whose low bits are the code; 0: slow path
    uint16_t dist_fast[1u << kDistFastBits];
    uint16_t lit_sym[288], dist_sym[32];    // symbols in canonical order
    uint16_t lit_count[16], dist_count[16]; // codes of each length
    uint16_t code[320];                     // per symbol (distances behind 288): its code, first bit lowest
    uint8_t lens[320];
    uint8_t in[kInWindow];
    uint32_t b_pos[kBatch];
    uint16_t b_len[kBatch], b_dist[kBatch]; // dist 0: the literal b_len; else length (bit 15: sync in front of this match)
    uint32_t nb, status, out_pos, win_base, final_block, eob, stored_src, stored_len, n_lit, n_dist;
};

struct HostCtx {
    static SVT_HD uint32_t lane() { return 0; }
    static SVT_HD uint32_t lanes() { return 1; }
    static SVT_HD void sync() {}
};

// ---- one BGZF member in `len` bytes at `off`: where its payload is, and its ISIZE; false: not a member that fits ------------
struct Member { uint64_t src; uint32_t clen, isize; uint64_t dst; };          // payload, and where its ISIZE bytes go
constexpr uint32_t kNoMember = 0xFFFFFFFFu;                                  // Member.isize of a member that cannot be used
SVT_HD bool member_at(const uint8_t* data, uint64_t len, uint64_t off, uint64_t& src, uint32_t& clen, uint32_t& isize, uint64_t& next)
{
    if (off > len || len - off < 18) return false;
    const uint8_t* h = data + off;
    if (h[0] != 31 || h[1] != 139) return false;
    const uint32_t xlen = h[10] | (h[11] << 8);
    if (len - off < 12ull + xlen) return false;
    int32_t bsize = -1;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint8_t* x = h + 12 + i;
        const uint32_t slen = x[2] | (x[3] << 8);
        if (x[0] == 66 && x[1] == 67 && i + 6 <= xlen) bsize = x[4] | (x[5] << 8);
        i += 4 + slen;
    }
    if (bsize < 0 || len - off < (uint64_t)bsize + 1) return false;
    const int32_t c = bsize - (int32_t)xlen - 19;
    if (c < 0) return false;
    const uint8_t* tail = h + 12 + xlen + c;
    src = off + 12 + xlen;
    clen = (uint32_t)c;
    isize = tail[4] | (tail[5] << 8) | (tail[6] << 16) | ((uint32_t)tail[7] << 24);
    next = off + (uint64_t)bsize + 1;
    return isize <= kMaxIsize;
}

// the CRC-32 its trailer stores for the member whose payload is data[src, src + clen) (member_at has vouched for the trailer's bytes)
SVT_HD uint32_t member_crc(const uint8_t* data, uint64_t src, uint32_t clen)
{
    const uint8_t* t = data + src + clen;
    return t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
}

// ---- lane 0's bit buffer over Scratch.in ---------------------------------------------------------------------------------------
struct Bits { uint64_t buf; uint32_t cnt, pos, clen; };     // `pos`: the next payload byte that goes into `buf`

SVT_HD void refill(const Scratch& S, Bits& B)
{
    while (B.cnt <= 56 && B.pos < B.clen && B.pos - S.win_base < kInWindow) {
        B.buf |= (uint64_t)S.in[B.pos - S.win_base] << B.cnt;
        B.cnt += 8;
        ++B.pos;
    }
}
SVT_HD bool need(const Scratch& S, Bits& B, uint32_t n)     // n <= 32
{
    if (B.cnt < n) refill(S, B);
    return B.cnt >= n;
}
SVT_HD uint32_t take(Bits& B, uint32_t n)
{
    const uint32_t v = (uint32_t)(B.buf & ((1ull << n) - 1));
    B.buf >>= n;
    B.cnt -= n;
    return v;
}

// one symbol of a canonical code, bit by bit (codes beyond the fast table, and the code-length code); < 0: -status
SVT_HD int32_t decode_slow(const Scratch& S, Bits& B, const uint16_t* count, const uint16_t* sym)
{
    refill(S, B);
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        if (len > B.cnt) return -(int32_t)INF_INPUT;
        code |= (int32_t)((B.buf >> (len - 1)) & 1);
        const int32_t c = count[len];
        if (code - c < first) {
            B.buf >>= len;
            B.cnt -= len;
            return sym[index + (code - first)];
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -(int32_t)INF_SYMBOL;
}
SVT_HD int32_t decode_fast(const Scratch& S, Bits& B, const uint16_t* fast, uint32_t fast_bits, const uint16_t* count, const uint16_t* sym)
{
    if (B.cnt < 15) refill(S, B);
    const uint32_t e = fast[B.buf & ((1u << fast_bits) - 1)];
    if (e) {
        const uint32_t len = e & 15;
        if (len > B.cnt) return -(int32_t)INF_INPUT;
        B.buf >>= len;
        B.cnt -= len;
        return (int32_t)(e >> 4);
    }
    return decode_slow(S, B, count, sym);
}

// counts, the subscription check of zlib's inflate_table, symbols in canonical order and every symbol's code (lane 0)
SVT_HD bool build_code(const uint8_t* lens, uint32_t n, uint16_t* count, uint16_t* sym, uint16_t* code, bool may_be_empty)
{
    for (uint32_t l = 0; l <= 15; ++l) count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++count[lens[s]];
    uint32_t max = 15;
    while (max > 0 && count[max] == 0) --max;
    if (max == 0) { count[0] = 0; return may_be_empty; }
    int32_t left = 1;
    for (uint32_t l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return false;
    }
    if (left > 0 && max != 1) return false;
    uint16_t offs[16], next[16];
    offs[1] = 0;
    next[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        next[l + 1] = (uint16_t)((next[l] + count[l]) << 1);
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s];
        if (!l) continue;
        sym[offs[l]++] = (uint16_t)s;
        uint32_t c = next[l]++, r = 0;
        for (uint32_t i = 0; i < l; ++i) { r = (r << 1) | (c & 1); c >>= 1; }
        code[s] = (uint16_t)r;
    }
    count[0] = 0;
    return true;
}

// block header and code lengths (lane 0); S.lens / S.n_lit / S.n_dist for a Huffman block, S.stored_* for a stored one
SVT_HD uint32_t read_block_header(Scratch& S, Bits& B, uint32_t isize)
{
    if (!need(S, B, 3)) return INF_INPUT;
    S.final_block = take(B, 1);
    const uint32_t type = take(B, 2);
    S.stored_len = 0xFFFFFFFFu;
    if (type == 3) return INF_BTYPE;
    if (type == 0) {
        take(B, B.cnt & 7);
        if (!need(S, B, 32)) return INF_INPUT;
        const uint32_t len = take(B, 16), nlen = take(B, 16);
        if ((len ^ 0xFFFFu) != nlen) return INF_STORED;
        const uint32_t src = B.pos - B.cnt / 8;            // (whole bytes are left in the buffer)
        if (len > B.clen - src) return INF_INPUT;
        if (len > isize - S.out_pos) return INF_OUTPUT;
        S.stored_src = src;
        S.stored_len = len;
        B.buf = 0;
        B.cnt = 0;
        B.pos = src + len;
        return INF_OK;
    }
    if (type == 1) {
        for (uint32_t s = 0; s < 288; ++s) S.lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        for (uint32_t s = 0; s < 32; ++s) S.lens[288 + s] = 5;
        S.n_lit = 288;
        S.n_dist = 32;
    } else {
        if (!need(S, B, 14)) return INF_INPUT;
        const uint32_t nlen = take(B, 5) + 257, ndist = take(B, 5) + 1, ncode = take(B, 4) + 4;
        if (nlen > 286 || ndist > 30) return INF_LENGTHS;
        static constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = 0; i < 19; ++i) S.lens[order[i]] = 0;
        for (uint32_t i = 0; i < ncode; ++i) {
            if (!need(S, B, 3)) return INF_INPUT;
            S.lens[order[i]] = (uint8_t)take(B, 3);
        }
        // (the code-length code borrows the distance tables: they are built behind it)
        if (!build_code(S.lens, 19, S.dist_count, S.dist_sym, S.code + 288, false)) return INF_LENGTHS;
        uint32_t have = 0;
        uint8_t* lens = S.lens;                            // (the 19 lengths are in the code's tables by now)
        while (have < nlen + ndist) {
            const int32_t sym = decode_slow(S, B, S.dist_count, S.dist_sym);
            if (sym < 0) return (uint32_t)-sym == INF_SYMBOL ? INF_LENGTHS : (uint32_t)-sym;
            if (sym < 16) { lens[have++] = (uint8_t)sym; continue; }
            uint32_t copy, len = 0;
            if (sym == 16) {
                if (have == 0) return INF_LENGTHS;
                if (!need(S, B, 2)) return INF_INPUT;
                len = lens[have - 1];
                copy = 3 + take(B, 2);
            } else if (sym == 17) {
                if (!need(S, B, 3)) return INF_INPUT;
                copy = 3 + take(B, 3);
            } else {
                if (!need(S, B, 7)) return INF_INPUT;
                copy = 11 + take(B, 7);
            }
            if (have + copy > nlen + ndist) return INF_LENGTHS;
            while (copy--) lens[have++] = (uint8_t)len;
        }
        // the distance lengths move up to 288 (nlen <= 286: from the top down nothing is overwritten before it is read)
        for (uint32_t s = ndist; s-- > 0;) S.lens[288 + s] = lens[nlen + s];
        if (S.lens[256] == 0) return INF_LENGTHS;
        S.n_lit = nlen;
        S.n_dist = ndist;
    }
    if (!build_code(S.lens, S.n_lit, S.lit_count, S.lit_sym, S.code, false)) return INF_LENGTHS;
    if (!build_code(S.lens + 288, S.n_dist, S.dist_count, S.dist_sym, S.code + 288, true)) return INF_LENGTHS;
    return INF_OK;
}

// up to kBatch symbols into S.b_* (lane 0); stops at the end of the block, at the end of the staged input, or with a status
SVT_HD uint32_t decode_batch(Scratch& S, Bits& B, uint32_t isize)
{
    uint32_t nb = 0, out_pos = S.out_pos, group = 0xFFFFFFFFu;
    S.eob = 0;
    while (nb < kBatch && B.pos - S.win_base + 8 <= kInWindow) {
        const int32_t sym = decode_fast(S, B, S.lit_fast, kFastBits, S.lit_count, S.lit_sym);
        if (sym < 0) return (uint32_t)-sym;
        if (sym < 256) {
            if (out_pos >= isize) return INF_OUTPUT;
            S.b_pos[nb] = out_pos++;
            S.b_len[nb] = (uint16_t)sym;
            S.b_dist[nb] = 0;
            ++nb;
            continue;
        }
        if (sym == 256) { S.eob = 1; break; }
        if (sym >= 286) return INF_SYMBOL;
        const uint32_t i = (uint32_t)sym - 257;
        uint32_t len = 258;
        if (i < 8) len = 3 + i;
        else if (i < 28) {
            const uint32_t e = i / 4 - 1;
            if (!need(S, B, e)) return INF_INPUT;
            len = 3 + ((4 + (i & 3)) << e) + take(B, e);
        }
        const int32_t ds = decode_fast(S, B, S.dist_fast, kDistFastBits, S.dist_count, S.dist_sym);
        if (ds < 0) return (uint32_t)-ds == INF_SYMBOL ? INF_DISTANCE : (uint32_t)-ds;
        if (ds >= 30) return INF_DISTANCE;
        uint32_t dist = 1 + (uint32_t)ds;
        if (ds >= 4) {
            const uint32_t e = (uint32_t)ds / 2 - 1;
            if (!need(S, B, e)) return INF_INPUT;
            dist = 1 + ((2 + ((uint32_t)ds & 1)) << e) + take(B, e);
        }
        if (dist > out_pos) return INF_DISTANCE;
        if (len > isize - out_pos) return INF_OUTPUT;
        // does it read what a match of this batch writes with no sync behind it yet?  (literals are all stored, and synced, first)
        const uint32_t src_end = out_pos - dist + (len < dist ? len : dist);
        uint32_t flag = 0;
        if (group != 0xFFFFFFFFu && src_end > group) { flag = 0x8000; group = out_pos; }
        else if (group == 0xFFFFFFFFu) group = out_pos;
        S.b_pos[nb] = out_pos;
        S.b_len[nb] = (uint16_t)(len | flag);
        S.b_dist[nb] = (uint16_t)dist;             // (<= 32 768: bit 15 alone is the largest distance)
        ++nb;
        out_pos += len;
    }
    S.nb = nb;
    S.out_pos = out_pos;
    return INF_OK;
}

template <class X>
SVT_HD void stage_input(Scratch& S, const uint8_t* cdata, uint32_t clen)
{
    const uint32_t base = S.win_base;
    for (uint32_t i = X::lane(); i < kInWindow; i += X::lanes()) S.in[i] = base + i < clen ? cdata[base + i] : 0;
}

template <class X>
SVT_HD void fill_fast(Scratch& S)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    for (uint32_t i = lane; i < (1u << kFastBits); i += lanes) S.lit_fast[i] = 0;
    for (uint32_t i = lane; i < (1u << kDistFastBits); i += lanes) S.dist_fast[i] = 0;
    X::sync();
    for (uint32_t s = lane; s < S.n_lit; s += lanes) {
        const uint32_t l = S.lens[s];
        if (l == 0 || l > kFastBits) continue;
        for (uint32_t k = S.code[s]; k < (1u << kFastBits); k += 1u << l) S.lit_fast[k] = (uint16_t)(s << 4 | l);
    }
    for (uint32_t s = lane; s < S.n_dist; s += lanes) {
        const uint32_t l = S.lens[288 + s];
        if (l == 0 || l > kDistFastBits) continue;
        for (uint32_t k = S.code[288 + s]; k < (1u << kDistFastBits); k += 1u << l) S.dist_fast[k] = (uint16_t)(s << 4 | l);
    }
    X::sync();
}

// the symbols of one batch into `out`: the literals, then the matches in order
template <class X>
SVT_HD void emit_batch(const Scratch& S, uint8_t* out)
{
    const uint32_t lane = X::lane(), lanes = X::lanes(), nb = S.nb;
    for (uint32_t k = lane; k < nb; k += lanes)
        if (S.b_dist[k] == 0) out[S.b_pos[k]] = (uint8_t)S.b_len[k];
    X::sync();
    for (uint32_t k = 0; k < nb; ++k) {
        const uint32_t dist = S.b_dist[k];
        if (!dist) continue;
        if (S.b_len[k] & 0x8000) X::sync();                 // (the same for every lane: it is read from Scratch)
        const uint32_t len = S.b_len[k] & 0x7FFF, pos = S.b_pos[k];
        const uint8_t* src = out + (pos - dist);
        if (dist >= len) for (uint32_t i = lane; i < len; i += lanes) out[pos + i] = src[i];
        else for (uint32_t i = lane; i < len; i += lanes) out[pos + i] = src[i % dist];
    }
    X::sync();
}

// The member's payload `cdata[clen]` into `out[isize]`.  The status is valid on every lane after the call; with a status other
// than INF_OK the bytes at `out` are not to be used.
template <class X>
SVT_HD uint32_t inflate_member(const uint8_t* cdata, uint32_t clen, uint8_t* out, uint32_t isize, Scratch& S)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    Bits B{0, 0, 0, clen};
    X::sync();                                             // (nobody still reads the Scratch of the member before)
    if (lane == 0) { S.status = isize <= kMaxIsize ? INF_OK : INF_MEMBER; S.out_pos = 0; S.final_block = 0; S.win_base = 0; S.nb = 0; }
    X::sync();
    // (every block takes three bits of input at least, every batch one symbol: both loops end with the input)
    while (S.status == INF_OK) {
        stage_input<X>(S, cdata, clen);
        X::sync();
        if (lane == 0) S.status = read_block_header(S, B, isize);
        X::sync();
        if (S.status != INF_OK) break;
        if (S.stored_len != 0xFFFFFFFFu) {
            const uint32_t n = S.stored_len, at = S.out_pos;
            const uint8_t* src = cdata + S.stored_src;
            for (uint32_t i = lane; i < n; i += lanes) out[at + i] = src[i];
            X::sync();
            if (lane == 0) { S.out_pos = at + n; S.win_base = B.pos; }
        } else {
            fill_fast<X>(S);
            for (;;) {
                if (lane == 0) S.win_base = B.pos;
                X::sync();
                stage_input<X>(S, cdata, clen);
                X::sync();
                if (lane == 0) {
                    const uint32_t st = decode_batch(S, B, isize);
                    if (st != INF_OK) { S.status = st; S.nb = 0; }
                }
                X::sync();
                if (S.status != INF_OK) break;
                emit_batch<X>(S, out);
                if (S.eob) break;
            }
            if (lane == 0) S.win_base = B.pos;
        }
        X::sync();
        if (S.status != INF_OK || S.final_block) break;
    }
    X::sync();
    if (lane == 0 && S.status == INF_OK && S.out_pos != isize) S.status = INF_SHORT;
    X::sync();
    return S.status;
}

}  // namespace inf
}  // namespace svt

#endif  // SVT_INFLATE_H

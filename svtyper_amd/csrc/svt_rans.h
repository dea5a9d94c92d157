// svt_rans.h -- rANS 4x8, the entropy coder of CRAM 3.0's block method 4 (CRAM format specification 3.0, section 13), order 0
// and order 1: the decoder.
//
// ONE piece of source for both places that run it, as svt_inflate.h and svt_crc32.h are: the host (svt_rans_decode_host: any
// C++17 compiler, where it is fuzzed and sanitised) and the device (svt_rans_kernel.h, hipcc).  What is written once: the block
// header (check_block), the frequency-table parser (parse_context, parse_order1) and the decode step of one state (advance,
// refill).  What each side writes for itself is the loop around the step: the host takes the four states one after the other,
// the kernel gives each state a lane.
//
// A block:  order (1 byte: 0 | 1), compressed size (u32 le: the bytes behind this header), uncompressed size (u32 le), then the
// frequency table, four u32 le states and the renormalisation bytes.
//
// Frequencies are 12 bits.  A table lists the symbols that occur in rising order, each `symbol, frequency` with the frequency
// in one byte below 128 and in two above; a symbol that follows its predecessor directly is followed by a count of further
// direct successors, which then come without their symbol byte; symbol byte 0 behind the first ends the table.  Order 1 wraps
// the same scheme around the contexts.  The frequencies of a context sum to 4096 -- or to 4095, which is what the encoder the
// format was published with writes: a state whose low twelve bits then say 4095 has no symbol (RANS_SYMBOL).
//
// Here the table of a context is kept as 257 cumulative frequencies C[0 .. 256] of 16 bits (C[s + 1] - C[s] is symbol s's
// frequency) and a state's symbol is found by an eight-step search in them: the largest s with C[s] <= m.  No 4096-entry
// reverse table is built (it would be filled byte by byte by the one lane that parses, and sixteen of them per wave are 64 KiB
// of LDS; profiles/rans_kernel_resources.txt).
//
// The renormalisation bytes are one stream the four states read from in state order.  After its advance a state is at least
// 2^11 (it was at least 2^23, a frequency is at least 1), so it needs 0, 1 or 2 bytes to be at least 2^23 again, and how many
// follows from the state alone (need()).  That is what lets four lanes share the stream: each computes its need, a prefix sum
// over the four gives its read offset and the stream's new position.  (A state of a damaged block may be below 2^11; it is
// given two bytes like any state below 2^15 -- what such a block decodes to is the same on both sides, and it is refused
// wherever the format can show the damage.)
//
// A block that is refused has its status set and its whole output range zeroed; nothing is read outside the block or written
// outside its output range, on either side: every read goes through In (bounds-checked) or is in front of a checked position.
// No std::, no allocation.
#ifndef SVT_RANS_H
#define SVT_RANS_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace rans {

constexpr uint32_t kTotBits = 12, kTot = 1u << kTotBits, kLow = 1u << 23;
constexpr uint32_t kHeader = 9;             // order, compressed size, uncompressed size
constexpr uint32_t kCtx = 257;              // cumulative entries of one context

enum Status : uint32_t {
    RANS_OK = 0,
    RANS_HEADER = 1,        // shorter than its header, an order other than 0 and 1, or sizes that are not the block's
    RANS_FREQ = 2,          // the frequency table runs out of the block, repeats itself or does not sum to 4096 (4095)
    RANS_INPUT = 3,         // the states or the renormalisation bytes run out of the block
    RANS_SYMBOL = 4,        // a state points at no symbol of its context
    RANS_SIZE = 5,          // order 1 with nothing to decode (the format has no such block)
};

// one block as the kernels take it: the bytes behind the header, where the output goes
struct Job { uint64_t in_off, out_off; uint32_t in_len, out_len, block, pad; };

SVT_HD uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The header of block[0, len) whose output is to be out_len bytes: its status, and its order.
SVT_HD uint32_t check_block(const uint8_t* block, uint64_t len, uint64_t out_len, uint32_t* order)
{
    *order = 0;
    if (len < kHeader || block[0] > 1) return RANS_HEADER;
    *order = block[0];
    if ((uint64_t)le32(block + 1) != len - kHeader || (uint64_t)le32(block + 5) != out_len) return RANS_HEADER;
    if (*order == 1 && out_len == 0) return RANS_SIZE;
    return RANS_OK;
}

// the bytes behind the header, read in order
struct In {
    const uint8_t* p;
    uint32_t at, end;
    bool bad;
    SVT_HD uint32_t get()
    {
        if (at >= end) { bad = true; return 0; }
        return p[at++];
    }
    SVT_HD uint32_t peek() const { return at < end ? p[at] : 0x100u; }
};

// One context's table from `in` into C[0 .. 256], which holds zeros.  False: malformed.
SVT_HD bool parse_context(In& in, uint16_t* C)
{
    uint32_t j = in.get(), rle = 0, x = 0;
    do {
        uint32_t f = in.get();
        if (f >= 128) f = ((f & 127) << 8) | in.get();
        if (in.bad || C[j + 1]) return false;           // (a symbol comes once)
        C[j + 1] = (uint16_t)f;
        x += f;
        if (x > kTot) return false;
        if (!rle && in.peek() == j + 1) {
            j = in.get();
            rle = in.get();
        } else if (rle) {
            --rle;
            if (++j > 255) return false;
        } else {
            j = in.get();
        }
        if (in.bad) return false;
    } while (j);
    if (x != kTot && x != kTot - 1) return false;
    uint32_t acc = 0;
    for (uint32_t s = 1; s <= 256; ++s) {
        acc += C[s];
        C[s] = (uint16_t)acc;
    }
    return true;
}

// The tables of the contexts that occur into C[256][257], which holds zeros.  False: malformed.
SVT_HD bool parse_order1(In& in, uint16_t* C)
{
    uint32_t i = in.get(), rle = 0;
    do {
        if (in.bad || C[i * kCtx + 256]) return false;   // (a context comes once: a parsed one ends in its sum)
        if (!parse_context(in, C + i * kCtx)) return false;
        if (!rle && in.peek() == i + 1) {
            i = in.get();
            rle = in.get();
        } else if (rle) {
            --rle;
            if (++i > 255) return false;
        } else {
            i = in.get();
        }
        if (in.bad) return false;
    } while (i);
    return true;
}

// what a state decodes to in its context, and the state behind it before it is refilled
struct Step { uint32_t sym, x; bool bad; };

SVT_HD Step advance(const uint16_t* C, uint32_t R)
{
    const uint32_t m = R & (kTot - 1);
    uint32_t s = 0;
#pragma unroll
    for (uint32_t step = 128; step; step >>= 1)
        if (C[s + step] <= m) s += step;
    const uint32_t lo = C[s], hi = C[s + 1];
    Step r;
    r.sym = s;
    r.bad = m >= hi;
    r.x = (hi - lo) * (R >> kTotBits) + m - lo;
    return r;
}

// the renormalisation bytes the state x takes: 0, 1 or 2
SVT_HD uint32_t need(uint32_t x) { return x >= kLow ? 0u : x >= (1u << 15) ? 1u : 2u; }

// x with its `n` bytes at p
SVT_HD uint32_t refill(uint32_t x, const uint8_t* p, uint32_t n)
{
    if (n) x = (x << 8) | p[0];
    if (n == 2) x = (x << 8) | p[1];
    return x;
}

// ---- the host's loop around the step ---------------------------------------------------------------------------------------

SVT_HD void zero_out(uint8_t* out, uint32_t out_len)
{
    for (uint32_t i = 0; i < out_len; ++i) out[i] = 0;
}

// The payload in[0, in_len) of a block of `order` into out[0, out_len), on one thread.  C: 257 entries for order 0, 256 x 257
// for order 1, all zero.  The block's header has passed check_block.
SVT_HD uint32_t decode_serial(uint32_t order, const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_len, uint16_t* C)
{
    if (out_len == 0) return RANS_OK;
    In r{in, 0, in_len, false};
    if (!(order ? parse_order1(r, C) : parse_context(r, C))) return RANS_FREQ;
    if (in_len - r.at < 16) return RANS_INPUT;
    uint32_t R[4], at = r.at + 16;
    for (uint32_t j = 0; j < 4; ++j) R[j] = le32(in + r.at + 4 * j);
    const uint32_t steps = out_len >> 2;
    uint32_t ctx[4] = {0, 0, 0, 0};
    for (uint32_t t = 0; t < steps; ++t) {
        Step st[4];
        uint32_t total = 0;
        bool bad = false;
        for (uint32_t j = 0; j < 4; ++j) {
            st[j] = advance(C + (order ? ctx[j] * kCtx : 0), R[j]);
            bad |= st[j].bad;
            total += need(st[j].x);
        }
        if (bad) return RANS_SYMBOL;
        if (total > in_len - at) return RANS_INPUT;
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t n = need(st[j].x);
            R[j] = refill(st[j].x, in + at, n);
            at += n;
            out[order ? j * steps + t : 4 * t + j] = (uint8_t)st[j].sym;
            ctx[j] = st[j].sym;
        }
    }
    if (!order) {                                        // the last 1 to 3 bytes: what the first states say, without an advance
        for (uint32_t j = 0; j < (out_len & 3); ++j) {
            const Step s = advance(C, R[j]);
            if (s.bad) return RANS_SYMBOL;
            out[4 * steps + j] = (uint8_t)s.sym;
        }
        return RANS_OK;
    }
    for (uint32_t i = 4 * steps; i < out_len; ++i) {     // order 1: the last quarter takes the remainder
        const Step s = advance(C + ctx[3] * kCtx, R[3]);
        if (s.bad) return RANS_SYMBOL;
        const uint32_t n = need(s.x);
        if (n > in_len - at) return RANS_INPUT;
        R[3] = refill(s.x, in + at, n);
        at += n;
        out[i] = (uint8_t)s.sym;
        ctx[3] = s.sym;
    }
    return RANS_OK;
}

}  // namespace rans
}  // namespace svt

#endif  // SVT_RANS_H

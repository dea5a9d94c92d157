// svt_dump_rules.h -- the evidence dump of `svtyper -w` from the walk's source rows: verdict bytes + the alignment records in the
// arena -> the BAM records the reference would have written.
//
// ONE piece of source for both places that run it: the host (svt_bam_evidence_dump_walk_host in svt_reads_walk.h, any C++17
// compiler; tests/native/asan_dump_rules_main.cpp runs it under AddressSanitizer) and the device (svt_dump_kernel.h).  Two rules:
//
//   (a) the decision per fragment -- driver.tag_and_write statement for statement (classic.py:296-413, parsers.py:771-782,
//       1218-1228).  A fragment is a row that is no continuation plus the continuation rows behind it; its primary reads are the
//       rec[0] / rec[1] of its rows, two SLOTS per row.  Every slot keeps a state {not set, R, A}:
//         1. an ungated is_ref_seq hit (SRC_HIT_A / SRC_HIT_B) sets R;
//         2. verdict bit 16 of row first + k sets A on the read behind seq candidate k, bit 32 on the read behind clip candidate k
//            (over R);
//         3. verdict bit 1 of the first row tags every primary that has no XV yet: A with bit 2, else R;
//         4. verdict bit 4 the same with bit 8.
//       "No XV yet": not set above AND no field named XV, of any type, in the record's tag area.  The fragment is written when
//       any of the four fired, and what is written is its primaries in order.
//   (b) the output record of one read -- what bam.AlignmentFile.write emits: the new block_size, bytes [0, 16) of the record,
//       four zero bytes (l_seq = 0; `bin` stays), bytes [20, 32 + l_read_name + 4 n_cigar), the tag area: unchanged for a read
//       that is not set, else without every field named XV and with 'X' 'V' 'A' 'R'|'A' behind the rest.
//
// Every access is bounded by the record's block_size and the arena's length.  Anything inconsistent -- a record that does not
// fit, a tag area rr::tag_field does not walk to its last byte, a verdict bit for a candidate the row does not have -- makes the
// unit "dump outside the envelope": it gets no bytes, its reads have to come from elsewhere.  Never guessed at.
//
// Execution: written once against a context `X` (X::lane() / X::lanes() / X::sync(), as svt_inflate.h and svt_crc32.h).
// size_unit deals fragments out to the lanes; place_slots is a prefix sum over the slots' lengths; emit_read copies one read
// with all lanes.  No atomics, no floats; what is written where depends on the rows and the verdicts only.
#ifndef SVT_DUMP_RULES_H
#define SVT_DUMP_RULES_H

#include <stdint.h>

#include "svt_evidence_walk.h"

namespace svt {
namespace dr {

using namespace rr;
using ew::SrcRow;
using ew::kNoRecord;

enum : uint8_t { XV_KEEP = 0, XV_R = 1, XV_A = 2, XV_STATE = 3, XV_IN_RECORD = 4 };   // a slot's state; XV_IN_RECORD only while a fragment is decided

// ---- one record -----------------------------------------------------------------------------------------------------------
struct Rec { const uint8_t* d; uint32_t size, body_end, tags_off; };   // d: behind block_size; the fixed part, name and CIGAR end at body_end
SVT_HD bool record_at(const uint8_t* arena, uint64_t arena_len, uint32_t off, Rec& r)
{
    if ((uint64_t)off + 4 > arena_len) return false;
    const uint32_t size = ld32(arena + off);
    if (size < 32 || size > ew::kMaxRecord || (uint64_t)off + 4 + size > arena_len) return false;
    Core c;
    if (!decode_core(arena + off + 4, size, c) || c.l_seq < 0) return false;
    r.d = arena + off + 4;
    r.size = size;
    r.body_end = 32 + c.l_name + 4 * c.n_cigar;
    r.tags_off = c.tags_off;
    return true;
}
SVT_HD bool is_xv(const uint8_t* field) { return field[0] == 'X' && field[1] == 'V'; }
// the bytes the fields named XV take; false: the tag area is not a run of whole fields up to the record's end
SVT_HD bool xv_bytes(const Rec& r, uint32_t& n)
{
    n = 0;
    uint32_t at = r.tags_off;
    for (;;) {                                             // (a field takes at least four bytes: at most size / 4 steps)
        uint32_t next = at;
        const uint32_t st = tag_field(r.d, r.size, at, next);
        if (st == TAGS_END) return at == r.size;
        if (st != TAG_FIELD) return false;
        if (is_xv(r.d + at)) n += next - at;
        at = next;
    }
}

// ---- one unit ---------------------------------------------------------------------------------------------------------------
struct Unit {
    const uint8_t* arena;
    uint64_t arena_len;
    const SrcRow* rows;        // the unit's n_rows source rows, in record order
    const uint8_t* verdicts;   // ... and verdict bytes (svt_batch_verdicts)
    uint32_t n_rows;
    uint32_t* slot_len;        // 2 * n_rows: the output length of row r's ra at 2 r, of its rb at 2 r + 1; 0 = not written
    uint8_t* slot_state;       // 2 * n_rows: XV_KEEP / XV_R / XV_A
};

// rule (a) for the fragment of rows [f, f + c); adds its output bytes to `bytes` and its written reads to `reads`; false: outside the envelope
SVT_HD bool size_fragment(const Unit& U, uint32_t f, uint32_t c, uint64_t& bytes, uint32_t& reads)
{
    bool any = false;
    for (uint32_t k = 0; k < c; ++k) {                    // 1. the slots as they are, and the ungated hits
        const SrcRow& row = U.rows[f + k];
        for (uint32_t j = 0; j < 2; ++j) {
            const uint32_t slot = 2 * (f + k) + j;
            U.slot_len[slot] = 0;
            U.slot_state[slot] = XV_KEEP;
            if (row.rec[j] == kNoRecord) continue;
            Rec r;
            uint32_t xv;
            if (!record_at(U.arena, U.arena_len, row.rec[j], r) || !xv_bytes(r, xv)) return false;
            const bool hit = (row.bits & (j ? ew::SRC_HIT_B : ew::SRC_HIT_A)) != 0;
            U.slot_len[slot] = 4 + r.body_end + (r.size - r.tags_off);
            U.slot_state[slot] = (uint8_t)((hit ? XV_R : XV_KEEP) | (xv ? XV_IN_RECORD : 0));
            any = any || hit;
        }
    }
    for (uint32_t k = 0; k < c; ++k) {                    // 2. the split candidates with p_alt > 0
        const uint8_t v = U.verdicts[f + k];
        for (uint32_t which = 2; which < 4; ++which) {
            if (!(v & (which == 2 ? 16u : 32u))) continue;
            const uint32_t off = U.rows[f + k].rec[which];
            if (off == kNoRecord) return false;
            bool found = false;
            for (uint32_t q = 0; q < 2 * c && !found; ++q)
                if (U.rows[f + q / 2].rec[q & 1] == off) {
                    U.slot_state[2 * f + q] = (uint8_t)((U.slot_state[2 * f + q] & XV_IN_RECORD) | XV_A);
                    found = true;
                }
            if (!found) return false;                     // (split.read is always a primary of its fragment)
            any = true;
        }
    }
    const uint8_t v0 = U.verdicts[f];
    for (uint32_t pass = 0; pass < 2; ++pass) {           // 3. tag_span(p_alt), 4. tag_span(1 - p_conc)
        if (!(v0 & (pass ? 4u : 1u))) continue;
        any = true;
        const uint8_t value = (v0 & (pass ? 8u : 2u)) ? XV_A : XV_R;
        for (uint32_t q = 0; q < 2 * c; ++q)
            if (U.slot_len[2 * f + q] && U.slot_state[2 * f + q] == XV_KEEP) U.slot_state[2 * f + q] = value;
    }
    for (uint32_t q = 0; q < 2 * c; ++q) {                // the lengths of what is written
        const uint32_t slot = 2 * f + q;
        const uint8_t state = U.slot_state[slot] & XV_STATE;
        U.slot_state[slot] = state;
        if (!any) { U.slot_len[slot] = 0; continue; }
        if (U.slot_len[slot] && state != XV_KEEP) {
            Rec r;
            uint32_t xv;
            if (!record_at(U.arena, U.arena_len, U.rows[f + q / 2].rec[q & 1], r) || !xv_bytes(r, xv)) return false;
            U.slot_len[slot] = U.slot_len[slot] - xv + 4;
        }
        bytes += U.slot_len[slot];
        reads += U.slot_len[slot] ? 1u : 0u;
    }
    return true;
}

// Launch 1: the fragments of a unit dealt out to the lanes.  Every lane returns ITS share of the unit's bytes and written reads and
// whether what it saw is inside the envelope: the caller adds the shares up and ands the answers.
template <class X>
SVT_HD bool size_unit(const Unit& U, uint64_t& bytes, uint32_t& reads)
{
    bytes = 0;
    reads = 0;
    bool ok = true;
    for (uint32_t f = X::lane(); f < U.n_rows; f += X::lanes()) {
        if (U.rows[f].bits & ew::SRC_CONTINUATION) {
            if (f == 0) ok = false;                        // (a unit begins with a fragment)
            continue;
        }
        uint32_t c = 1;
        while (f + c < U.n_rows && (U.rows[f + c].bits & ew::SRC_CONTINUATION)) ++c;
        if (ok && !size_fragment(U, f, c, bytes, reads)) ok = false;
    }
    return ok;
}

// Launch 2, first half: slot_off[k] = the sum of slot_len[0 .. k).  `partial`: X::lanes() words of scratch.
template <class X>
SVT_HD void place_slots(const uint32_t* slot_len, uint32_t* slot_off, uint32_t n, uint32_t* partial)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const uint32_t per = (n + lanes - 1) / lanes;
    const uint32_t b = (uint64_t)lane * per < n ? lane * per : n, e = b + per < n ? b + per : n;
    uint32_t sum = 0;
    for (uint32_t k = b; k < e; ++k) sum += slot_len[k];
    X::sync();                                             // (nobody still reads the partial sums of the unit before)
    partial[lane] = sum;
    X::sync();
    if (lane == 0) {
        uint32_t run = 0;
        for (uint32_t l = 0; l < lanes; ++l) { const uint32_t mine = partial[l]; partial[l] = run; run += mine; }
    }
    X::sync();
    uint32_t run = partial[lane];
    for (uint32_t k = b; k < e; ++k) { slot_off[k] = run; run += slot_len[k]; }
    X::sync();
}

// dword copies where source and destination agree mod 4, bytes elsewhere; the lanes of X side by side
template <class X>
SVT_HD void copy_bytes(uint8_t* dst, const uint8_t* src, uint32_t n)
{
    const uint32_t lane = X::lane(), lanes = X::lanes();
    if ((((uintptr_t)dst ^ (uintptr_t)src) & 3u) != 0 || n < 8) {
        for (uint32_t i = lane; i < n; i += lanes) dst[i] = src[i];
        return;
    }
    const uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u), words = (n - head) / 4;
    for (uint32_t i = lane; i < head; i += lanes) dst[i] = src[i];
    const uint8_t* s = static_cast<const uint8_t*>(__builtin_assume_aligned(src + head, 4));
    uint8_t* d = static_cast<uint8_t*>(__builtin_assume_aligned(dst + head, 4));
    for (uint32_t i = lane; i < words; i += lanes) {       // (a word through memcpy: one dword load and store, and no aliasing question)
        uint32_t w;
        __builtin_memcpy(&w, s + 4 * i, 4);
        __builtin_memcpy(d + 4 * i, &w, 4);
    }
    for (uint32_t i = head + 4 * words + lane; i < n; i += lanes) dst[i] = src[i];
}

// Launch 2, second half -- rule (b): the read whose block_size word lies at `off`, in `state`, into dst[0 .. len), `len` being
// what size_fragment found for it.  Nothing is written beyond `len`; false (and an undefined dst) when the record does not give
// exactly `len` bytes -- which it does unless the arena changed between the launches.
template <class X>
SVT_HD bool emit_read(const uint8_t* arena, uint64_t arena_len, uint32_t off, uint8_t state, uint8_t* dst, uint32_t len)
{
    Rec r;
    if (!record_at(arena, arena_len, off, r) || len < 4 + r.body_end) return false;
    const uint32_t lane = X::lane(), lanes = X::lanes();
    const uint32_t block_size = len - 4;
    for (uint32_t i = lane; i < 4; i += lanes) dst[i] = (uint8_t)(block_size >> (8 * i));
    copy_bytes<X>(dst + 4, r.d, 16);
    for (uint32_t i = lane; i < 4; i += lanes) dst[20 + i] = 0;
    copy_bytes<X>(dst + 24, r.d + 20, r.body_end - 20);
    uint32_t o = 4 + r.body_end;
    if (state == XV_KEEP) {
        if (len - o != r.size - r.tags_off) return false;
        copy_bytes<X>(dst + o, r.d + r.tags_off, r.size - r.tags_off);
        return true;
    }
    uint32_t at = r.tags_off, run = at;                    // [run, at): fields that stay, not copied yet
    for (;;) {
        uint32_t next = at;
        const uint32_t st = tag_field(r.d, r.size, at, next);
        const bool end = st != TAG_FIELD, drop = !end && is_xv(r.d + at);
        if (end || drop) {
            if (at - run > len - o) return false;
            copy_bytes<X>(dst + o, r.d + run, at - run);
            o += at - run;
            run = next;
        }
        if (end) {
            if (st != TAGS_END || at != r.size) return false;
            break;
        }
        at = next;
    }
    if (len - o != 4) return false;
    if (lane == 0) { dst[o] = 'X'; dst[o + 1] = 'V'; dst[o + 2] = 'A'; dst[o + 3] = state == XV_A ? 'A' : 'R'; }
    return true;
}

}  // namespace dr
}  // namespace svt

#endif  // SVT_DUMP_RULES_H

// Audit of the sync marks of svt_inflate.h on the CPU.  decode_batch sets bit 15 of b_len on a match whose source a match of the
// same batch has written with no barrier behind it; on the device that mark is all that orders the loads of one lane behind the
// stores of another, on the host (one lane, sync() is nothing) a missing mark changes nothing a test of the bytes could see.
//
// This program drives the header's own functions in the order inflate_member uses them (stage_input, read_block_header, fill_fast,
// decode_batch, emit_batch<HostCtx>) and, behind every decode_batch, checks the property itself by brute force, without the
// decoder's `group` reasoning: walk the batch's matches in order; a marked match empties the per-byte set "written by a match
// since the last barrier"; a match's source bytes [pos - dist, pos - dist + min(len, dist)) must not meet that set; the match
// then adds [pos, pos + len).  (The literals of a batch are all stored, and followed by a barrier, before its first match.)
//
//   inflate_marks IN OUT [--erase]
// IN:  per stream u32 label length, label, u32 payload length, u32 isize, payload (raw deflate, no BGZF wrapper: a payload may
//      be larger than a member holds).   OUT: per stream u32 status, u32 n, n bytes (n = isize when the status is 0, else 0).
// One line per stream on stdout: label, status, status of inflate_member<HostCtx>, whether the bytes of the two are equal,
// batches, matches, marked, violations, and the marks the brute force finds unnecessary (information: they may be conservative).
// --erase: the self-check.  Every batch's marks are erased before the audit, which then has to report violations wherever a
// mark was needed.
// Built and run by tests/test_inflate_marks.py with g++.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "svt_inflate.h"

using namespace svt::inf;

struct Audit { uint64_t batches = 0, matches = 0, marked = 0, violations = 0, unnecessary = 0; };

static std::vector<uint32_t> g_stamp(kMaxIsize + 1, 0);        // byte -> the epoch a match wrote it in
static uint32_t g_epoch = 0;

static void audit_batch(const Scratch& S, uint32_t isize, Audit& a)
{
    ++a.batches;
    ++g_epoch;                                                 // (emit_batch ends with a barrier, and has one behind the literals)
    for (uint32_t k = 0; k < S.nb; ++k) {
        const uint32_t dist = S.b_dist[k];
        if (!dist) continue;
        const uint32_t len = S.b_len[k] & 0x7FFF, pos = S.b_pos[k];
        const bool marked = (S.b_len[k] & 0x8000) != 0;
        if (dist > pos || len > isize - pos) { ++a.violations; continue; }        // (decode_batch checked both)
        const uint32_t src = pos - dist, n = len < dist ? len : dist;
        bool meets = false;
        for (uint32_t i = 0; i < n; ++i) meets |= g_stamp[src + i] == g_epoch;
        ++a.matches;
        if (marked) {
            ++a.marked;
            if (!meets) ++a.unnecessary;
            ++g_epoch;
        } else if (meets) {
            ++a.violations;
        }
        for (uint32_t i = 0; i < len; ++i) g_stamp[pos + i] = g_epoch;
    }
}

// inflate_member<HostCtx>, step for step, with the audit between decode_batch and emit_batch
static uint32_t drive(const uint8_t* cdata, uint32_t clen, uint8_t* out, uint32_t isize, Scratch& S, Audit& a, bool erase)
{
    Bits B{0, 0, 0, clen};
    S.status = isize <= kMaxIsize ? INF_OK : INF_MEMBER;
    S.out_pos = 0; S.final_block = 0; S.win_base = 0; S.nb = 0;
    while (S.status == INF_OK) {
        stage_input<HostCtx>(S, cdata, clen);
        S.status = read_block_header(S, B, isize);
        if (S.status != INF_OK) break;
        if (S.stored_len != 0xFFFFFFFFu) {
            std::memcpy(out + S.out_pos, cdata + S.stored_src, S.stored_len);
            S.out_pos += S.stored_len;
            S.win_base = B.pos;
        } else {
            fill_fast<HostCtx>(S);
            for (;;) {
                S.win_base = B.pos;
                stage_input<HostCtx>(S, cdata, clen);
                const uint32_t st = decode_batch(S, B, isize);
                if (st != INF_OK) { S.status = st; S.nb = 0; break; }
                if (erase) for (uint32_t k = 0; k < S.nb; ++k) if (S.b_dist[k]) S.b_len[k] &= 0x7FFF;
                audit_batch(S, isize, a);
                emit_batch<HostCtx>(S, out);
                if (S.eob) break;
            }
            S.win_base = B.pos;
        }
        if (S.status != INF_OK || S.final_block) break;
    }
    if (S.status == INF_OK && S.out_pos != isize) S.status = INF_SHORT;
    return S.status;
}

static bool get(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: inflate_marks IN OUT [--erase]\n"); return 2; }
    const bool erase = argc > 3 && std::string(argv[3]) == "--erase";
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* outf = std::fopen(argv[2], "wb");
    if (!in || !outf) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    std::unique_ptr<Scratch> S(new Scratch()), S2(new Scratch());
    uint32_t nl = 0;
    while (get(in, &nl, 4)) {
        std::string label(nl, ' ');
        uint32_t clen = 0, isize = 0;
        if (!get(in, &label[0], nl) || !get(in, &clen, 4) || !get(in, &isize, 4)) return 3;
        std::vector<uint8_t> payload(clen);
        if (clen && !get(in, payload.data(), clen)) return 3;
        const uint32_t room = isize <= kMaxIsize ? isize : 0;
        std::vector<uint8_t> a_out(room + 1, 0xA5), b_out(room + 1, 0xA5);     // (one byte behind: nothing may be written there)
        Audit a;
        const uint32_t st = drive(payload.data(), clen, a_out.data(), isize, *S, a, erase);
        const uint32_t st2 = inflate_member<HostCtx>(payload.data(), clen, b_out.data(), isize, *S2);
        const bool same = st == st2 && (st != INF_OK || std::memcmp(a_out.data(), b_out.data(), room) == 0) && a_out[room] == 0xA5 && b_out[room] == 0xA5;
        std::printf("%s\t%u\t%u\t%d\t%llu\t%llu\t%llu\t%llu\t%llu\n", label.c_str(), st, st2, same ? 1 : 0, (unsigned long long)a.batches,
                    (unsigned long long)a.matches, (unsigned long long)a.marked, (unsigned long long)a.violations, (unsigned long long)a.unnecessary);
        const uint32_t n = st == INF_OK ? room : 0;
        std::fwrite(&st, 4, 1, outf);
        std::fwrite(&n, 4, 1, outf);
        if (n) std::fwrite(a_out.data(), 1, n, outf);
    }
    std::fclose(in);
    std::fclose(outf);
    return 0;
}

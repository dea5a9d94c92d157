// asan_cram_main.cpp -- the rANS 4x8 host twin (svt_rans.h, svt_rans_batch.h) and the CRAM slice decoder (svt_cram.h) over a
// corpus the test writes, in a program of its own that is built with -fsanitize=address,undefined
// (tests/test_cram_native.py).  Every buffer is a heap block of exactly its size, so a read or write past it is seen.
//
// Lines of the corpus:
//   R <block hex | -> <output size> <status wanted | -1> <output hex wanted | ->
//   S <compression header hex> <slice header hex> <n_ref> <read group ids, comma separated | -> <records wanted | -1>
//     <n blocks> { <content id> <core 0|1> <content hex | -> }
// An S line that wants -1 records may be refused or not; what it must not do is touch memory it does not own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "svt_cram.h"
#include "svt_rans_batch.h"

static std::vector<uint8_t> unhex(const std::string& s)
{
    std::vector<uint8_t> out;
    if (s == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)(v(s[i]) << 4 | v(s[i + 1])));
    return out;
}

// a heap block of exactly the vector's size (a vector's capacity may hide a read behind its end)
struct Exact {
    uint8_t* p;
    size_t n;
    explicit Exact(const std::vector<uint8_t>& v) : p(new uint8_t[v.size() ? v.size() : 1]), n(v.size())
    {
        if (n) std::memcpy(p, v.data(), n);
    }
    Exact(const Exact&) = delete;
    ~Exact() { delete[] p; }
};

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    long rans = 0, slices = 0, refused = 0;
    while (std::getline(in, line)) {
        std::istringstream f(line);
        std::string kind;
        f >> kind;
        if (kind == "R") {
            std::string block_hex, want_hex;
            uint64_t out_size;
            long want_status;
            f >> block_hex >> out_size >> want_status >> want_hex;
            const std::vector<uint8_t> block = unhex(block_hex), want = unhex(want_hex);
            Exact data(block);
            constexpr uint64_t kGuard = 8;
            std::vector<uint8_t> image(out_size + 2 * kGuard, 0xA5);
            Exact out(image);
            const uint64_t off[2] = {0, data.n}, out_off[1] = {kGuard}, sizes[1] = {out_size};
            uint32_t status[1] = {99};
            std::vector<svt::rans::Job> o0, o1;
            if (svt::rans::plan_batch(data.p, data.n, off, 1, out_off, sizes, out.p, out.n, status, o0, o1) != 0) {
                std::printf("plan_batch refused its arguments: %s\n", svt::g_err.c_str());
                return 1;
            }
            for (int order = 0; order < 2; ++order)
                for (const auto& j : order ? o1 : o0) {
                    std::vector<uint16_t> zero(order ? 256 * svt::rans::kCtx : svt::rans::kCtx, 0);
                    uint16_t* C = new uint16_t[zero.size()];
                    std::memcpy(C, zero.data(), zero.size() * sizeof(uint16_t));
                    const uint32_t st = svt::rans::decode_serial((uint32_t)order, data.p + j.in_off, j.in_len, out.p + j.out_off, j.out_len, C);
                    if (st != svt::rans::RANS_OK) svt::rans::zero_out(out.p + j.out_off, j.out_len);
                    status[j.block] = st;
                    delete[] C;
                }
            for (uint64_t i = 0; i < kGuard; ++i)
                if (out.p[i] != 0xA5 || out.p[kGuard + out_size + i] != 0xA5) {
                    std::printf("rANS case %ld: a guard byte was written\n", rans);
                    return 1;
                }
            if (want_status >= 0 && status[0] != (uint32_t)want_status) {
                std::printf("rANS case %ld: status %u, wanted %ld\n", rans, status[0], want_status);
                return 1;
            }
            if (want_status == 0 && (want.size() != out_size || (out_size && std::memcmp(out.p + kGuard, want.data(), out_size) != 0))) {
                std::printf("rANS case %ld: the bytes differ\n", rans);
                return 1;
            }
            ++rans;
        } else if (kind == "S") {
            std::string comp_hex, sl_hex, rg_text;
            int n_ref;
            long want_records;
            size_t n_blocks;
            f >> comp_hex >> sl_hex >> n_ref >> rg_text >> want_records >> n_blocks;
            const std::vector<uint8_t> comp_v = unhex(comp_hex), sl_v = unhex(sl_hex);
            Exact comp(comp_v), sl(sl_v);
            std::vector<std::string> rg;
            if (rg_text != "-") {
                std::istringstream r(rg_text);
                std::string id;
                while (std::getline(r, id, ',')) rg.push_back(id);
            }
            std::vector<std::unique_ptr<Exact>> held;
            std::vector<svt::cram::Block> blocks;
            for (size_t k = 0; k < n_blocks; ++k) {
                int cid, core;
                std::string hex;
                f >> cid >> core >> hex;
                held.emplace_back(new Exact(unhex(hex)));
                blocks.push_back(svt::cram::Block{held.back()->p, held.back()->n, cid, core != 0});
            }
            std::vector<uint8_t> records;
            std::vector<uint64_t> rec_off;
            try {
                svt::cram::decode_slice(comp.p, comp.n, sl.p, sl.n, blocks, rg, n_ref, records, rec_off);
                if (want_records >= 0 && (long)rec_off.size() - 1 != want_records) {
                    std::printf("slice case %ld: %zu records, wanted %ld\n", slices, rec_off.size() - 1, want_records);
                    return 1;
                }
                // every record lies inside the bytes and says its own size
                for (size_t k = 0; k + 1 < rec_off.size(); ++k) {
                    int32_t size;
                    std::memcpy(&size, records.data() + rec_off[k], 4);
                    if (rec_off[k + 1] > records.size() || (uint64_t)size + 4 != rec_off[k + 1] - rec_off[k]) {
                        std::printf("slice case %ld: record %zu does not fit its block_size\n", slices, k);
                        return 1;
                    }
                }
            } catch (const svt::cram::Refuse& e) {
                if (want_records >= 0) {
                    std::printf("slice case %ld: refused (%s)\n", slices, e.what());
                    return 1;
                }
                ++refused;
            }
            ++slices;
        }
    }
    std::printf("rans %ld slices %ld refused %ld\n", rans, slices, refused);
    return 0;
}

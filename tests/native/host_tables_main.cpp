// host_tables_main.cpp -- build_tables (svtyper_amd/csrc/svt_host_tables.h) on libraries read from a file, one call per library,
// for tests/test_concordance_host.py.
//
//   host_tables <in> <out>
//
// in:  uint32 n_libs, then per library  int32 key_min, uint32 n_bins, double mean, double sd, uint32 hist[n_bins]
// out: per library  int32 rc, uint32 narrow_bins, uint32 fast_geometry, uint32 n (= n_bins + 1, 0 when rc != 0),
//      then n times {int32 thr, uint32 hist} -- the library's bins as the device gets them, the sentinel last
// stdout: one line per library: index, rc, narrow_bins, fast_geometry, n
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "svt_host_tables.h"

static bool read_all(std::FILE* f, void* p, size_t n) { return std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) {
        std::fprintf(stderr, "cannot open the files\n");
        return 2;
    }
    uint32_t n_libs = 0;
    if (!read_all(in, &n_libs, 4)) return 3;
    for (uint32_t l = 0; l < n_libs; ++l) {
        int32_t key_min = 0;
        uint32_t n_bins = 0;
        double mean = 0, sd = 0;
        if (!read_all(in, &key_min, 4) || !read_all(in, &n_bins, 4) || !read_all(in, &mean, 8) || !read_all(in, &sd, 8)) return 3;
        std::vector<uint32_t> hist(n_bins);
        if (n_bins && !read_all(in, hist.data(), (size_t)n_bins * 4)) return 3;
        svt_library lib{};
        lib.hist = hist.data();
        lib.key_min = key_min;
        lib.n_bins = n_bins;
        lib.mean = mean;
        lib.sd = sd;
        svt_evidence_batch batch{};
        batch.n_libs = 1;
        batch.libs = &lib;
        batch.split_weight = 1.0;
        batch.disc_weight = 1.0;
        svt::HostTables T;
        const int32_t rc = svt::build_tables(&batch, 1, T);
        const uint32_t head[3] = {T.narrow_bins ? 1u : 0u, T.fast_geometry ? 1u : 0u, rc == SVT_OK ? (uint32_t)T.bins.size() : 0u};
        std::fwrite(&rc, 4, 1, out);
        std::fwrite(head, 4, 3, out);
        if (head[2]) std::fwrite(T.bins.data(), sizeof(svt::Bin), head[2], out);
        std::printf("%u\t%d\t%u\t%u\t%u\n", l, rc, head[0], head[1], head[2]);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}

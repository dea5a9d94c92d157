// svt_rans_batch.h -- what svt_rans_decode_host and svt_rans_decode_device (include/svtyper_reads.h) ask of their arguments, and
// the batch as jobs: once, for both translation units of the library.  Block k is data[off[k], off[k + 1]) and decodes to
// out[out_off[k], out_off[k] + out_size[k]); the output ranges may leave gaps (a caller's guard bytes) and may not overlap the
// end of `out`.  A block whose header is refused (rans::check_block) gets its status here, its output range is zeroed, and it
// is no job.
#ifndef SVT_RANS_BATCH_H
#define SVT_RANS_BATCH_H

#include <cstring>
#include <vector>

#include "../../include/svtyper_hip.h"
#include "svt_error.h"
#include "svt_rans.h"

namespace svt {
namespace rans {

inline int plan_batch(const uint8_t* data, uint64_t data_len, const uint64_t* off, uint64_t n, const uint64_t* out_off, const uint64_t* out_size,
                      uint8_t* out, uint64_t out_len, uint32_t* status, std::vector<Job>& order0, std::vector<Job>& order1)
{
    if (n && (!off || !out_off || !out_size || !status)) return fail(SVT_ERR_INVALID, "svt_rans_decode: null argument");
    if ((data_len && !data) || (out_len && !out)) return fail(SVT_ERR_INVALID, "svt_rans_decode: null argument");
    if (n > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "svt_rans_decode: too many blocks in one call (< 2^32)");
    for (uint64_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k] || off[k + 1] > data_len) return fail(SVT_ERR_INVALID, "svt_rans_decode: off must rise and stay inside data");
        if (out_off[k] > out_len || out_size[k] > out_len - out_off[k]) return fail(SVT_ERR_INVALID, "svt_rans_decode: an output range outside out");
        if (off[k + 1] - off[k] > 0xFFFFFFFFull || out_size[k] > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "svt_rans_decode: a block of 4 GiB or more");
    }
    order0.clear();
    order1.clear();
    for (uint64_t k = 0; k < n; ++k) {
        uint32_t order = 0;
        status[k] = check_block(data + off[k], off[k + 1] - off[k], out_size[k], &order);
        if (status[k] != RANS_OK) {
            if (out_size[k]) std::memset(out + out_off[k], 0, out_size[k]);
            continue;
        }
        const Job j{off[k] + kHeader, out_off[k], (uint32_t)(off[k + 1] - off[k] - kHeader), (uint32_t)out_size[k], (uint32_t)k, 0};
        (order ? order1 : order0).push_back(j);
    }
    return SVT_OK;
}

}  // namespace rans
}  // namespace svt

#endif  // SVT_RANS_BATCH_H

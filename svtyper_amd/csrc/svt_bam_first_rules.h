// svt_bam_first_rules.h -- first occurrences of a BAM record stream: the key of a record and when two keys are the same one
// (include/svtyper_reads.h: svt_bam_first_host / _device).
//
// ONE piece of source for both places that run the rule, as svt_bam_sort_rules.h and svt_dump_rules.h are: key_of, key_equal and
// key_hash are compiled for the host (svt_bam_first_host, any C++17 compiler: this is where they are proven against the
// restatement of tests/bamfirstcases.py and sanitised) and for the device (svt_bam_first_kernel.h, one lane per record).  The
// key is what driver._write_dumped reads: the l_read_name - 1 name bytes at offset 36 and the 16-bit flag at offset 18.  A
// record is read through its key alone, and a key is made by key_of alone, which checks every offset against the record's own
// span (never only against the stream's length); no std::, no allocation.  The host twin of the whole pass stands below it.
#ifndef SVT_BAM_FIRST_RULES_H
#define SVT_BAM_FIRST_RULES_H

#include <stdint.h>

#include "svt_geometry_math.h"

namespace svt {
namespace bfr {

constexpr uint32_t kFixed = 36;                 // block_size and the 32 bytes behind it
constexpr uint32_t kNameAt = 36, kFlagAt = 18, kNameLenAt = 12;

// the key of a well-formed record: name[0, len) lies inside the record's span
struct Key {
    const uint8_t* name;
    uint32_t len;                               // l_read_name - 1: the name without its NUL
    uint32_t flag;
};

// the record p[0, avail) (block_size first) -> its key; false for a record that is not well-formed: a span below 36 bytes, a
// block_size that is not the span's length less 4, l_read_name = 0, or a name that runs past the span
SVT_HD bool key_of(const uint8_t* p, uint64_t avail, Key& k)
{
    k.name = p;
    k.len = 0;
    k.flag = 0;
    if (avail < kFixed) return false;
    const uint64_t block_size = (uint64_t)p[0] | ((uint64_t)p[1] << 8) | ((uint64_t)p[2] << 16) | ((uint64_t)p[3] << 24);
    if (block_size != avail - 4) return false;
    const uint32_t l_read_name = p[kNameLenAt];
    if (l_read_name < 1 || (uint64_t)kNameAt + l_read_name > avail) return false;
    k.name = p + kNameAt;
    k.len = l_read_name - 1;
    k.flag = (uint32_t)p[kFlagAt] | (uint32_t)p[kFlagAt + 1] << 8;
    return true;
}

// record i of bytes[0, len) by the offset table (n + 1 entries): a span that the table does not keep inside the bytes has no key
SVT_HD bool key_at(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t i, Key& k)
{
    const uint64_t at = rec_off[i], next = rec_off[i + 1];
    if (at <= next && next <= len) return key_of(bytes + at, next - at, k);
    k.name = bytes;
    k.len = 0;
    k.flag = 0;
    return false;
}

// same flag, same length, same bytes
SVT_HD bool key_equal(const Key& a, const Key& b)
{
    if (a.flag != b.flag || a.len != b.len) return false;
    for (uint32_t c = 0; c < a.len; ++c)
        if (a.name[c] != b.name[c]) return false;
    return true;
}

// FNV-1a (64 bits) over p[0, n), from `h` on: also the hash of a VCF line's ID (svt_vcf_group.h)
SVT_HD uint64_t fnv1a(const uint8_t* p, uint32_t n, uint64_t h = 0xcbf29ce484222325ull)
{
    for (uint32_t c = 0; c < n; ++c) h = (h ^ p[c]) * 0x100000001b3ull;
    return h;
}

// FNV-1a over the name bytes, then the flag's two bytes, low byte first
SVT_HD uint64_t key_hash(const Key& k)
{
    uint64_t h = fnv1a(k.name, k.len);
    h = (h ^ (k.flag & 255u)) * 0x100000001b3ull;
    h = (h ^ (k.flag >> 8 & 255u)) * 0x100000001b3ull;
    return h;
}

// the low `hash_bits` bits (1..64) of a hash: what the device sorts by (fewer than 64 bits make distinct keys collide: tests)
SVT_HD uint64_t hash_mask(uint32_t hash_bits) { return hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1; }

}  // namespace bfr
}  // namespace svt

// ------------------------------------------------------------------------------------------ host code
#include <unordered_set>

namespace svt {
namespace bfr {

struct KeyHasher {
    size_t operator()(const Key& k) const { return (size_t)key_hash(k); }
};
struct KeySame {
    bool operator()(const Key& a, const Key& b) const { return key_equal(a, b); }
};

// svt_bam_first_host without its argument checks: keep[i] = 1 iff no record in front of i has i's key; -> the 1-based number of the
// first record that is not well-formed (keep is then undefined), or 0 with n_kept = the sum of keep
inline uint64_t first_host(const uint8_t* bytes, uint64_t len, const uint64_t* rec_off, uint64_t n, uint8_t* keep, uint64_t& n_kept)
{
    n_kept = 0;
    std::unordered_set<Key, KeyHasher, KeySame> seen;           // views into `bytes`
    seen.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i) {
        Key k;
        if (!key_at(bytes, len, rec_off, i, k)) return i + 1;
        keep[i] = seen.insert(k).second ? 1 : 0;
        n_kept += keep[i];
    }
    return 0;
}

}  // namespace bfr
}  // namespace svt
#endif  // SVT_BAM_FIRST_RULES_H

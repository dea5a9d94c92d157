// svt_reads_records.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): one BAM
// alignment (Record), its tag walk, the next record off a Bgzf, the pysam-style fetch.  Needs: Bgzf (svt_bgzf_reader.h), svt_bam
// (svt_reads_handle.h).
namespace {

// One BAM alignment: the fixed fields (rr::Core) and the record's bytes -- inside the inflated block, or the caller's gather
// buffer for a record that straddles blocks: valid until the next record is read.
struct Record : rr::Core {
    const uint8_t* data = nullptr;
    uint32_t size = 0;
    const char* name() const { return reinterpret_cast<const char*>(data + 32); }
    uint32_t name_len() const { return l_name ? l_name - 1 : 0; }
    const uint8_t* cigar() const { return data + 32 + l_name; }     // n_cigar words
    int64_t tlen() const { return (int32_t)rr::ld32(data + 28); }   // template_length
    std::string name_str() const { return std::string(name(), name_len()); }
};

// The first leg of a kept read's tag walk (svtyper_amd/bam.py::_parse_tags): up to its RG value, noting an SA value met on the
// way.  nullptr: no usable RG tag.  A read that becomes a split candidate walks on from `at` (tags_behind_rg); every other
// kept read stops here.  A value that runs over the record's end ends the walk without a complaint (rr::TAGS_OVERRUN).
const char* read_group(const Record& r, rr::Tags& t, uint32_t& at)
{
    rr::tags_begin(t);
    at = r.tags_off;
    if (rr::walk_tags(r.data, r.size, at, /*stop_at_rg=*/true, t) != rr::TAGS_AT_RG) return nullptr;
    return reinterpret_cast<const char*>(r.data + t.rg_off);
}
// The second leg: every tag behind RG is validated (a malformed tag anywhere fails the call, as bam.py raises:
// tests/test_native_reads.py::test_truncated_tag_behind_rg_is_malformed_in_both_tag_orders) and the first SA value noted.
bool tags_behind_rg(const Record& r, rr::Tags& t, uint32_t at)
{
    return rr::walk_tags(r.data, r.size, at, false, t) != rr::TAGS_MALFORMED;
}

// The bytes of the next alignment (after its length word): in place inside the inflated block when the
// record does not straddle a block boundary -- no copy, which is what makes walking up to a window cheap
// -- otherwise gathered into `buf`.  nullptr at the end of the data / on a bad length.
const uint8_t* next_record(Bgzf& z, std::vector<uint8_t>& buf, uint32_t& size)
{
    constexpr uint32_t kMaxRecord = 1u << 28;   // no alignment record is a quarter of a gigabyte: a corrupt length
    if (const uint8_t* h = z.contiguous(4)) {
        size = ld32(h);
        if (size < 32 || size > kMaxRecord) { z.mark_bad(); return nullptr; }
        if (const uint8_t* d = z.contiguous(4 + (size_t)size)) {
            z.advance(4 + (size_t)size);
            return d + 4;
        }
    }
    uint8_t szb[4];
    if (z.read(szb, 4) != 4) return nullptr;
    size = ld32(szb);
    if (size < 32 || size > kMaxRecord) { z.mark_bad(); return nullptr; }
    buf.resize(size);
    if (z.read(buf.data(), size) != size) return nullptr;
    return buf.data();
}

// fixed fields + reference end: all a fetch needs to decide whether the record overlaps its window
bool decode(const uint8_t* d, uint32_t size, Record& r)
{
    r.data = d;
    r.size = size;
    return d && rr::decode_core(d, size, r);
}

bool read_record(Bgzf& z, std::vector<uint8_t>& buf, Record& r)
{
    uint32_t size = 0;
    const uint8_t* d = next_record(z, buf, size);
    return decode(d, size, r);
}

// the merged index chunks a fetch of [beg, end) on `tid` walks, in file order (scratch of the calling thread)
const std::vector<std::pair<uint64_t, uint64_t>>& fetch_chunks(const svt_bam& bam, int32_t tid, int64_t beg, int64_t end)
{
    // (reused from fetch to fetch: two fetches per unit, three allocations each)
    static thread_local std::vector<uint32_t> bins;
    static thread_local std::vector<std::pair<uint64_t, uint64_t>> chunks, merged;
    bam.index.fetch_chunks(tid, beg, end, bam.ref_lengths[tid], bins, chunks, merged);
    return merged;
}

// pysam-style fetch: records with pos < end and reference end > beg, in file order; `fn` returns
// false to stop.  Mirrors svtyper_amd/bam.py::AlignmentFile.fetch.
template <typename Fn>
bool fetch(const svt_bam& bam, Bgzf& z, int32_t tid, int64_t beg, int64_t end, std::vector<uint8_t>& buf, Fn&& fn)
{
    if (tid < 0 || tid >= (int32_t)bam.ref_names.size()) return false;
    beg = std::max<int64_t>(beg, 0);
    if (end <= beg) return true;
    const auto& merged = fetch_chunks(bam, tid, beg, end);
    if (merged.empty()) return true;
    Record r;
    for (const auto& c : merged) {
        z.seek(c.first);
        while (z.tell() < c.second) {
            uint32_t size = 0;
            const uint8_t* d = next_record(z, buf, size);
            if (!decode(d, size, r)) break;
            // (verify: a fetch that ends early has still read through a block whose CRC-32 did not match)
            if (r.tid != tid || r.pos >= end) return !z.crc_failed();
            int64_t rend = r.end;
            if (r.n_cigar == 0 || rend <= r.pos) rend = (int64_t)r.pos + 1;
            if (rend > beg && !fn(r)) return !z.crc_failed();      // (most records walked on the way to the window stop here)
        }
    }
    return !z.failed();
}

}  // namespace

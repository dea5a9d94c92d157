// svt_bgzf_reader.h -- part of the translation unit svt_reads.cpp (included there, behind its other includes; not a stand-alone
// header): the BGZF layer of the native reader.  The mapped file, the per-thread library decoder, the step that verifies one
// inflated member, the blocks shared between a call's workers, the random-access reader Bgzf -- and the definitions of what
// svt_bgzf.h declares for both translation units: the CRC helpers, bgzf_members and the one host loop over a MemberSet.
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <condition_variable>

namespace {

// ------------------------------------------------------------------------------------------
// BGZF: random access through (compressed offset << 16 | in-block offset) addresses
// ------------------------------------------------------------------------------------------
// the whole file, mapped read-only once per handle and shared by all worker threads: no read()
// syscalls or stdio buffers on the fetch path, the inflate input is the mapping itself
struct FileMap {
    const uint8_t* data = nullptr;
    size_t size = 0;
    FileMap() = default;
    FileMap(const FileMap&) = delete;
    FileMap& operator=(const FileMap&) = delete;
    ~FileMap() { if (data) munmap(const_cast<uint8_t*>(data), size); }
    bool open(const std::string& path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size <= 0) { ::close(fd); return false; }
        void* p = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_SHARED, fd, 0);
        ::close(fd);
        if (p == MAP_FAILED) return false;
        madvise(p, (size_t)st.st_size, MADV_RANDOM);   // region fetches, not a scan
        data = static_cast<const uint8_t*>(p);
        size = (size_t)st.st_size;
        return true;
    }
};

// Raw-deflate decoding of BGZF blocks is where a region fetch spends its time on real data (a window is reached by
// inflating every block from the start of its 16-kb bin).  libdeflate's whole-buffer decoder is 2-3x faster
// than zlib's streaming one; the image ships its runtime (libdeflate.so.0) without headers, so it is bound by
// name at first use and zlib stays as the decoder when it is absent (or SVT_INFLATE=zlib asks for it).
struct FastInflate {
    void* (*alloc)() = nullptr;
    int (*decompress)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    void (*release)(void*) = nullptr;
    uint32_t (*crc)(uint32_t, const void*, size_t) = nullptr;   // verify: libdeflate_crc32, when the library has it
    FastInflate()
    {
        const char* want = std::getenv("SVT_INFLATE");
        if (want && std::strcmp(want, "zlib") == 0) return;
        void* h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        crc = reinterpret_cast<uint32_t (*)(uint32_t, const void*, size_t)>(dlsym(h, "libdeflate_crc32"));
        alloc = reinterpret_cast<void* (*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
        decompress = reinterpret_cast<int (*)(void*, const void*, size_t, void*, size_t, size_t*)>(
            dlsym(h, "libdeflate_deflate_decompress"));
        release = reinterpret_cast<void (*)(void*)>(dlsym(h, "libdeflate_free_decompressor"));
        if (!alloc || !decompress || !release) alloc = nullptr;
    }
    bool usable() const { return alloc != nullptr; }
};
static const FastInflate& fast_inflate()
{
    static const FastInflate f;
    return f;
}

// The library decoder of one thread: a libdeflate decompressor, or a zlib stream that is reset per member when fast_inflate()
// has none.  The one place that sets either up.
class HostInflater {
public:
    HostInflater() : fast_(fast_inflate().usable() ? fast_inflate().alloc() : nullptr)
    {
        std::memset(&zs_, 0, sizeof zs_);
        if (!fast_) zs_ok_ = inflateInit2(&zs_, -15) == Z_OK;
    }
    ~HostInflater() { if (fast_) fast_inflate().release(fast_); else if (zs_ok_) inflateEnd(&zs_); }
    HostInflater(const HostInflater&) = delete;
    HostInflater& operator=(const HostInflater&) = delete;
    bool ok() const { return fast_ || zs_ok_; }
    // the raw deflate stream cdata[0, clen) to exactly `isize` bytes at `out`; false: it does not inflate to that
    bool inflate(const uint8_t* cdata, uint32_t clen, uint8_t* out, uint32_t isize)
    {
        if (isize == 0) return true;
        if (fast_) return fast_inflate().decompress(fast_, cdata, clen, out, isize, nullptr) == 0;   // (null "actual size": a short stream fails)
        if (!zs_ok_ || inflateReset(&zs_) != Z_OK) return false;
        zs_.next_in = const_cast<Bytef*>(cdata);
        zs_.avail_in = (uInt)clen;
        zs_.next_out = out;
        zs_.avail_out = (uInt)isize;
        return ::inflate(&zs_, Z_FINISH) == Z_STREAM_END && zs_.avail_out == 0;
    }

private:
    void* const fast_;       // libdeflate's decompressor, or null: zlib's stream
    z_stream zs_;
    bool zs_ok_ = false;
};

// What one thread has verified, until it is added to the handle's tally.
struct VerifyCounts {
    uint64_t verified = 0, failed = 0;
    double crc_s = 0.0;
    void flush(svt::VerifyTally* tally) { if (tally && verified) tally->add(verified, failed, crc_s, 0.0); }
};
// Verify one member that has inflated to out[0, isize): its CRC-32 (the one-source code with a scratch `one_source`, else
// host_crc32) is timed, compared with the trailer's `stored` and counted.  inf::INF_OK or inf::INF_CRC.
uint32_t verify_member(const uint8_t* out, uint32_t isize, uint32_t stored, svt::crc::Scratch* one_source, VerifyCounts& n, uint32_t* computed = nullptr)
{
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t crc = one_source ? svt::crc::crc_member<svt::crc::HostCtx>(out, isize, svt::crc_tables(), *one_source) : svt::host_crc32(out, isize);
    n.crc_s += svt::seconds_since(t0);
    ++n.verified;
    if (computed) *computed = crc;
    if (crc == stored) return svt::inf::INF_OK;
    ++n.failed;
    return svt::inf::INF_CRC;
}

std::string crc_mismatch_text(uint64_t coff, uint32_t stored, uint32_t computed)
{
    char text[128];
    std::snprintf(text, sizeof text, "BGZF block at offset %llu: CRC32 mismatch (stored 0x%08x, computed 0x%08x)", (unsigned long long)coff, stored, computed);
    return text;
}

// One inflated BGZF block: immutable once it is published, so readers on several threads can hold it.
struct BlockData {
    std::vector<uint8_t> data;
    uint64_t next = 0;         // compressed offset of the block behind it (== its own offset: end of data / unusable block)
};
typedef std::shared_ptr<const BlockData> BlockRef;

// Inflated blocks shared by the worker threads of ONE svt_bam_summarise call.  Workers take runs of neighbouring units,
// and a worker that starts a run walks up to its first window through the blocks in front of it (a window is reached from
// the start of its 16-kb bin: seven 64-KiB blocks at 30x on average) -- blocks the worker of the run before inflates too,
// for its own last units.  Measured on 290 whole-genome-like sites: 24 % (8 workers) to 54 % (15) of all inflate calls were
// such repeats, and inflate is three quarters of the reader's time there.  A block is looked up here after the reader's own
// slots missed and published after it was inflated: one short critical section per 64 KiB of records.  64 shards x 16 ways
// = 1 024 blocks (64 MiB) at most, first-in-first-out per shard; a block a reader still holds outlives its eviction.
class SharedBlocks {
public:
    // The block at `coff`, or null with *claimed = true: the caller inflates it and then calls publish() or abandon().
    // While one worker inflates a block the others that want it wait here instead of inflating it too (workers start
    // their runs side by side: with 47 of them 2 291 inflate calls for 929 blocks before this).
    // With `in_flight` the call does not wait: a block somebody else is inflating comes back as null, *in_flight = true.
    BlockRef find_or_claim(uint64_t coff, bool* claimed, bool* in_flight = nullptr)
    {
        Shard& sh = shard(coff);
        std::unique_lock<std::mutex> g(sh.lock);
        *claimed = false;
        if (in_flight) *in_flight = false;
        for (;;) {
            int at = -1;
            for (int i = 0; i < kWays; ++i)
                if (sh.coff[i] == coff) { at = i; break; }
            if (at >= 0 && sh.block[at]) return sh.block[at];
            if (at < 0) {                                    // nobody has it, nobody is on it: the caller's
                sh.coff[sh.clock] = coff;
                sh.block[sh.clock].reset();
                sh.clock = (sh.clock + 1) % kWays;
                *claimed = true;
                return BlockRef();
            }
            if (in_flight) {
                *in_flight = true;
                return BlockRef();
            }
            sh.ready.wait(g);                                // in flight: published, abandoned or pushed out when we wake
        }
    }
    void publish(uint64_t coff, const BlockRef& b)
    {
        Shard& sh = shard(coff);
        {
            std::lock_guard<std::mutex> g(sh.lock);
            int at = -1;
            for (int i = 0; i < kWays; ++i)
                if (sh.coff[i] == coff) { at = i; break; }
            if (at < 0) {                                    // (its place went to sixteen newer blocks meanwhile)
                at = sh.clock;
                sh.clock = (sh.clock + 1) % kWays;
                sh.coff[at] = coff;
            }
            sh.block[at] = b;
        }
        sh.ready.notify_all();
    }
    void abandon(uint64_t coff)                              // the block is unusable: whoever waits finds that out for itself
    {
        Shard& sh = shard(coff);
        {
            std::lock_guard<std::mutex> g(sh.lock);
            for (int i = 0; i < kWays; ++i)
                if (sh.coff[i] == coff && !sh.block[i]) sh.coff[i] = ~0ull;
        }
        sh.ready.notify_all();
    }

private:
    static constexpr int kShards = 64, kWays = 16;
    struct Shard {
        std::mutex lock;
        std::condition_variable ready;
        uint64_t coff[kWays];
        BlockRef block[kWays];                               // null under a valid offset: being inflated
        int clock = 0;
        Shard() { for (auto& c : coff) c = ~0ull; }
    };
    Shard& shard(uint64_t coff) { return shards_[(coff * 0x9E3779B97F4A7C15ull) >> 58]; }
    Shard shards_[kShards];
};

class Bgzf {
public:
    // `verify` (svt_bam_set_verify; null: off): every block this reader inflates has its CRC-32 checked, and is counted there
    explicit Bgzf(const FileMap& file, SharedBlocks* shared = nullptr, svt::VerifyTally* verify = nullptr)
        : file_(file), shared_(shared), verify_(verify), empty_(std::make_shared<BlockData>())
    {
        block_ = empty_.get();
    }
    ~Bgzf() { verified_.flush(verify_); }
    Bgzf(const Bgzf&) = delete;
    Bgzf& operator=(const Bgzf&) = delete;
    bool ok() const { return file_.data != nullptr && decoder_.ok(); }
    bool failed() const { return bad_; }
    void mark_bad() { bad_ = true; }   // the record stream inside the blocks is corrupt
    // verify: a block this reader inflated did not have the CRC-32 its trailer stores (it is failed() too); the text for the caller
    bool crc_failed() const { return !crc_error_.empty(); }
    const std::string& crc_error() const { return crc_error_; }
    uint64_t n_inflated = 0, n_shared_hits = 0, n_ahead = 0;   // (SVT_TRACE)
    double inflate_s = 0.0;
    // when set: every block this reader loads is noted here (the arena of svt_bam_evidence_device is put together from them)
    std::vector<std::pair<uint64_t, BlockRef>>* touched = nullptr;

    void seek(uint64_t voff)
    {
        load(voff >> 16);
        uoff_ = (size_t)(voff & 0xFFFF);
    }
    uint64_t tell() const
    {
        if (uoff_ >= block_->data.size() && !block_->data.empty()) return block_->next << 16;
        return (coff_ << 16) | uoff_;
    }
    // The position as it stands, where tell() carries the end of a block over to the start of the next.  Behind a read: the block
    // that holds the last byte read, and the offset behind that byte.
    void last_read(uint64_t* coff, uint32_t* end) const { *coff = coff_; *end = (uint32_t)uoff_; }
    // after seek(): an offset behind the bytes of a block that has none (tell() reports it as it is; the next read starts in the
    // block behind it)
    bool offset_in_empty_block() const { return uoff_ > 0 && block_->data.empty(); }
    // returns the number of bytes actually read
    size_t read(void* dst, size_t n)
    {
        size_t got = 0;
        uint8_t* out = static_cast<uint8_t*>(dst);
        while (got < n) {
            const size_t avail = block_->data.size() - std::min(uoff_, block_->data.size());
            if (avail == 0) {
                const uint64_t next = block_->next;
                if (block_ != empty_.get() && next == coff_) break;
                if (!load(next)) break;
                uoff_ = 0;
                continue;
            }
            const size_t take = std::min(avail, n - got);
            std::memcpy(out + got, block_->data.data() + uoff_, take);
            uoff_ += take;
            got += take;
        }
        return got;
    }

    // n bytes at the read position as one span inside the current inflated block, or nullptr when they
    // straddle a block boundary / the file ends (the caller then falls back to read()).  The pointer stays
    // valid until the next call that may load a block.
    const uint8_t* contiguous(size_t n)
    {
        if (uoff_ >= block_->data.size()) {
            const uint64_t next = block_->next;
            if (block_ != empty_.get() && next == coff_) return nullptr;
            if (!load(next)) return nullptr;
            uoff_ = 0;
        }
        return block_->data.size() - uoff_ >= n ? block_->data.data() + uoff_ : nullptr;
    }
    void advance(size_t n) { uoff_ += n; }   // over bytes contiguous() has just vouched for

private:
    // Recently used blocks of this reader: the two windows of a unit and its neighbours walk forward through the same
    // blocks, and a list of sites often comes back to a region (both ends of a large event, overlapping calls, the same
    // targets again).  kSlots references, 8 MiB of blocks at most; the offsets sit in an array of their own: a look-up is
    // one pass over 1 KiB.  (32 slots: a cycle over ~50 blocks -- the fixture's 211 sites, repeated -- missed on every
    // third site, a third of the reader's time.)
    static constexpr int kSlots = 128;
    int slot_for(uint64_t coff) const
    {
        for (int i = 0; i < n_slots_; ++i)
            if (coffs_[i] == coff) return i;
        return -1;
    }
    bool use(uint64_t coff, const BlockRef& b)           // make `b` the current block, remembered under `coff`
    {
        int i;
        if (n_slots_ < kSlots) i = n_slots_++;
        else {
            i = clock_;
            clock_ = (clock_ + 1) % kSlots;
        }
        coffs_[i] = coff;
        slots_[i] = b;
        block_ = b.get();
        coff_ = coff;
        if (touched) touched->emplace_back(coff, b);
        return !block_->data.empty() || block_->next > coff;
    }
    bool park(uint64_t coff, bool is_bad)                // end of file / unusable block: an empty block that is its own successor
    {
        if (is_bad) bad_ = true;
        auto b = std::make_shared<BlockData>();
        b->next = coff;
        use(coff, b);
        return false;
    }
    // The block at `coff` inflated into a fresh BlockData; null with *unusable = false at the end of the file, null with
    // *unusable = true for a header that cannot be one.  A stream that does not inflate still returns its block (the
    // bytes stay readable) with *unusable = true.
    std::shared_ptr<BlockData> inflate_block(uint64_t coff, bool* unusable)
    {
        *unusable = false;
        if (coff + 18 > file_.size) return nullptr;                    // end of file
        *unusable = true;
        uint64_t src = 0, next = 0;
        uint32_t clen = 0, isize = 0;
        if (!svt::inf::member_at(file_.data, file_.size, coff, src, clen, isize, next)) return nullptr;
        const uint8_t* cdata = file_.data + src;
        auto b = std::make_shared<BlockData>();
        b->data.resize(isize);
        b->next = next;
        const auto t_inflate = std::chrono::steady_clock::now();
        bool inflated = decoder_.inflate(cdata, clen, b->data.data(), isize);
        inflate_s += svt::seconds_since(t_inflate);
        ++n_inflated;
        if (verify_ && inflated) {                       // a mismatch is a block that does not inflate, with a text of its own
            const uint32_t stored = svt::inf::member_crc(cdata, 0, clen);
            uint32_t computed = 0;
            if (verify_member(b->data.data(), isize, stored, nullptr, verified_, &computed) != svt::inf::INF_OK) {
                inflated = false;
                if (crc_error_.empty()) crc_error_ = crc_mismatch_text(coff, stored, computed);
            }
        }
        *unusable = !inflated;
        return b;
    }
    // offset of the block behind the one at `coff`, from its header alone; 0 when there is none to be had
    uint64_t next_offset(uint64_t coff) const
    {
        uint64_t src = 0, next = 0;
        uint32_t clen = 0, isize = 0;
        return svt::inf::member_at(file_.data, file_.size, coff, src, clen, isize, next) ? next : 0;
    }
    struct Claim {                                       // a claimed block that is not published is given up on every way out
        SharedBlocks* shared = nullptr;
        uint64_t coff = 0;
        ~Claim() { if (shared) shared->abandon(coff); }
    };
    // Somebody else is inflating the block this reader needs next.  Readers walk forward, so the blocks behind it are
    // wanted too -- by this reader, and by the one it waits for: instead of waiting, inflate the first of the next
    // kAhead blocks nobody has or is on.  Workers that walk up to neighbouring windows through the same blocks thereby
    // inflate them side by side instead of queueing behind one another (47 workers on 290 whole-genome-like sites spent
    // two thirds of their time in that queue).  False when there was nothing to do.
    bool help_ahead(uint64_t coff)
    {
        static constexpr int kAhead = 12;
        uint64_t c = coff;
        for (int k = 0; k < kAhead; ++k) {
            c = next_offset(c);
            if (c == 0 || c + 18 > file_.size) return false;
            if (slot_for(c) >= 0) continue;
            bool claimed = false, in_flight = false;
            if (shared_->find_or_claim(c, &claimed, &in_flight) || in_flight) continue;
            Claim claim{shared_, c};
            bool unusable = false;
            std::shared_ptr<BlockData> b = inflate_block(c, &unusable);
            if (!b || unusable) return false;            // (left to the reader that gets there: it reports the failure)
            shared_->publish(c, b);
            claim.shared = nullptr;
            ++n_ahead;
            return true;
        }
        return false;
    }
    bool load(uint64_t coff)
    {
        const int hit = slot_for(coff);
        if (hit >= 0) {
            block_ = slots_[hit].get();
            coff_ = coff;
            return !block_->data.empty() || block_->next > coff;
        }
        Claim claim;
        if (shared_) {
            for (;;) {
                bool claimed = false, in_flight = false;
                if (BlockRef b = shared_->find_or_claim(coff, &claimed, &in_flight)) { ++n_shared_hits; return use(coff, b); }
                if (claimed) { claim.shared = shared_; claim.coff = coff; break; }
                if (help_ahead(coff)) continue;          // (in flight elsewhere: useful work first, then look again)
                if (BlockRef b = shared_->find_or_claim(coff, &claimed)) { ++n_shared_hits; return use(coff, b); }   // waits
                if (claimed) { claim.shared = shared_; claim.coff = coff; }
                break;
            }
        }
        bool unusable = false;
        std::shared_ptr<BlockData> b = inflate_block(coff, &unusable);
        if (!b) return park(coff, unusable);
        if (unusable) bad_ = true;                       // (its bytes stay readable, as before: the caller sees failed())
        if (claim.shared && !unusable) { shared_->publish(coff, b); claim.shared = nullptr; }
        use(coff, b);
        return true;
    }

    const FileMap& file_;
    SharedBlocks* shared_;
    svt::VerifyTally* verify_;
    VerifyCounts verified_;  // (added to the tally when this reader goes)
    std::string crc_error_;
    HostInflater decoder_;   // one decoder per reader
    BlockRef slots_[kSlots];
    uint64_t coffs_[kSlots];
    int n_slots_ = 0;
    int clock_ = 0;
    std::shared_ptr<BlockData> empty_;
    const BlockData* block_ = nullptr;
    uint64_t coff_ = 0;
    size_t uoff_ = 0;
    bool bad_ = false;
};

}  // namespace

namespace svt {

uint32_t host_crc32(const uint8_t* p, size_t n)
{
    if (fast_inflate().crc) return fast_inflate().crc(0, p, n);
    return (uint32_t)::crc32(0L, p, (uInt)n);              // (n <= 65 536)
}

// the tables of svt_crc32.h for both translation units' callers
const crc::Tables& crc_tables()
{
    static const crc::Tables* const T = [] { auto* t = new crc::Tables(); crc::fill_tables(*t); return t; }();
    return *T;
}

// the arguments of svt_bgzf_crc32_host / _device
int crc_check_offsets(const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint32_t* crc)
{
    if (n && (!off || !crc)) return fail(SVT_ERR_INVALID, "null argument");
    if (n > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "svt_bgzf_crc32: too many members in one call (< 2^32)");
    for (uint64_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return fail(SVT_ERR_INVALID, "svt_bgzf_crc32: off must not decrease");
        if (off[k + 1] - off[k] > crc::kMaxLen) return fail(SVT_ERR_INVALID, "svt_bgzf_crc32: a member has at most 65536 bytes");
    }
    if (n && off[n] && !bytes) return fail(SVT_ERR_INVALID, "null argument");
    return SVT_OK;
}

// the arguments of svt_bgzf_deflate_host / _device
int deflate_check_args(const uint8_t* bytes, const uint64_t* off, uint64_t n, const uint8_t* out, const uint64_t* out_off, uint64_t& slots)
{
    slots = 0;
    if (!off || !out_off || (n && !out)) return fail(SVT_ERR_INVALID, "null argument");
    if (n > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: too many members in one call (< 2^32)");
    for (uint64_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: off must not decrease");
        if (off[k + 1] - off[k] > dfl::kMaxPayload) return fail(SVT_ERR_INVALID, "svt_bgzf_deflate: a payload has at most 65280 bytes");
        slots += dfl::slot_bytes((uint32_t)(off[k + 1] - off[k]));
    }
    if (n && off[n] > off[0] && !bytes) return fail(SVT_ERR_INVALID, "null argument");
    return SVT_OK;
}

int huffman_check_args(const uint32_t* freq, uint32_t sets, uint32_t symbols, uint32_t limit, const uint8_t* lengths)
{
    if (sets && (!freq || !lengths)) return fail(SVT_ERR_INVALID, "null argument");
    if (limit != 7 && limit != 15) return fail(SVT_ERR_INVALID, "svt_huffman_lengths: limit is 7 or 15");
    if (symbols < 1 || symbols > dfl::kLitSyms) return fail(SVT_ERR_INVALID, "svt_huffman_lengths: 1 .. 286 symbols");
    for (uint64_t k = 0; k < sets; ++k) {
        uint64_t sum = 0, used = 0;
        for (uint32_t s = 0; s < symbols; ++s) { sum += freq[k * symbols + s]; used += freq[k * symbols + s] != 0; }
        if (sum > 0xFFFFFFFFull) return fail(SVT_ERR_INVALID, "svt_huffman_lengths: the frequencies of a histogram sum to 2^32 or more");
        if (used > (1ull << limit)) return fail(SVT_ERR_INVALID, "svt_huffman_lengths: more used symbols than codes of `limit` bits");
    }
    return SVT_OK;
}

namespace bgzf {

int bgzf_members(const uint8_t* data, uint64_t len, const uint64_t* block_off, uint64_t n, const uint8_t* out, const uint64_t* out_off,
                 const uint32_t* status, MemberSet& set)
{
    set = MemberSet();
    if (n && (!status || (!out && out_off && out_off[n]))) return fail(SVT_ERR_INVALID, "null argument");
    if ((!data && len) || (n && (!block_off || !out_off))) return fail(SVT_ERR_INVALID, "null argument");
    set.file = data;
    set.file_size = set.compressed_bytes = len;
    set.spans.push_back(MemberSet::Span{0, len, 0});
    set.arena_bytes = n ? out_off[n] : 0;
    set.members.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
        if (out_off[k + 1] < out_off[k]) return fail(SVT_ERR_INVALID, "svt_bgzf_inflate: out_off must not decrease");
        uint64_t src = 0, next = 0;
        uint32_t clen = 0, isize = 0;
        const bool ok = inf::member_at(data, len, block_off[k], src, clen, isize, next) && out_off[k + 1] - out_off[k] == isize;
        set.members[k] = inf::Member{ok ? src : 0, ok ? clen : 0, ok ? isize : inf::kNoMember, out_off[k]};
    }
    return SVT_OK;
}

void inflate_members_host(const MemberSet& set, uint8_t* dst, unsigned n_threads, Decoder decoder, Crc crc, VerifyTally* verify,
                          std::vector<uint32_t>& status)
{
    const size_t m = set.members.size();
    status.assign(m, inf::INF_OK);
    std::atomic<size_t> next(0);
    run_threads(std::max(1u, n_threads), [&](unsigned) {
        const std::unique_ptr<inf::Scratch> S(decoder == Decoder::one_source ? new inf::Scratch() : nullptr);
        const std::unique_ptr<HostInflater> library(decoder == Decoder::library ? new HostInflater() : nullptr);
        const std::unique_ptr<svt::crc::Scratch> C(verify && crc == Crc::one_source ? new svt::crc::Scratch() : nullptr);
        VerifyCounts verified;
        for (;;) {
            const size_t k0 = next.fetch_add(8);
            if (k0 >= m) break;
            for (size_t k = k0; k < std::min(m, k0 + 8); ++k) {
                const inf::Member& mb = set.members[k];
                if (mb.isize == inf::kNoMember) { status[k] = inf::INF_MEMBER; continue; }
                const uint8_t* cdata = set.payload(mb);
                uint8_t* out = dst + mb.dst;
                if (S) status[k] = inf::inflate_member<inf::HostCtx>(cdata, mb.clen, out, mb.isize, *S);
                else status[k] = library->inflate(cdata, mb.clen, out, mb.isize) ? inf::INF_OK : inf::INF_INPUT;
                if (verify && status[k] == inf::INF_OK) status[k] = verify_member(out, mb.isize, inf::member_crc(cdata, 0, mb.clen), C.get(), verified);
            }
        }
        verified.flush(verify);
    });
}

}  // namespace bgzf
}  // namespace svt

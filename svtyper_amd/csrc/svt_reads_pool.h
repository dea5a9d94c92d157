// svt_reads_pool.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the gather's
// huge-page buffers (BufferPool, SummaryArena), a thread's CPU clock, svt_reads_trim.  Needs: no other part.
namespace {

// Large host buffers of the summariser (the workers' arenas, the flat summary array): anonymous mappings advised for
// transparent huge pages -- the summaries are written once and read once, so what they cost is page faults and, when they
// go, the unmapping: on the 2 x EPYC 9575F box 17 ms to unmap the arenas of 2.1 M summaries and as much again for the
// flat array, a third of the call.  Mappings therefore go back to a process-wide pool (at most SVT_READER_POOL_MB, default
// 1024, of idle memory; 0 = unmap at once) and the next call starts on pages that are already there.
class BufferPool {
public:
    static BufferPool& get()
    {
        static BufferPool* pool = new BufferPool();      // (never destroyed: buffers may be returned during process exit)
        return *pool;
    }
    // a mapping of at least `bytes` (its real size goes to *cap), nullptr when the system has none
    void* acquire(size_t bytes, size_t* cap)
    {
        const size_t want = (std::max<size_t>(bytes, 1) + kGrain - 1) / kGrain * kGrain;
        {
            std::lock_guard<std::mutex> g(lock_);
            size_t best = idle_.size();
            for (size_t i = 0; i < idle_.size(); ++i)    // smallest idle mapping that fits and is not more than twice too big
                if (idle_[i].second >= want && idle_[i].second <= 2 * want && (best == idle_.size() || idle_[i].second < idle_[best].second)) best = i;
            if (best != idle_.size()) {
                void* p = idle_[best].first;
                *cap = idle_[best].second;
                idle_bytes_ -= *cap;
                idle_.erase(idle_.begin() + (long)best);
                return p;
            }
        }
        void* p = mmap(nullptr, want, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return nullptr;
        madvise(p, want, MADV_HUGEPAGE);
        *cap = want;
        return p;
    }
    void release(void* p, size_t cap)
    {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(lock_);
            if (idle_bytes_ + cap <= limit_) {
                idle_.emplace_back(p, cap);
                idle_bytes_ += cap;
                return;
            }
        }
        munmap(p, cap);
    }
    // the flat array handed to the caller: its size is remembered here so that svt_summaries_free needs only the pointer
    void* acquire_tracked(size_t bytes)
    {
        size_t cap = 0;
        void* p = acquire(bytes, &cap);
        if (p) {
            std::lock_guard<std::mutex> g(lock_);
            lent_[p] = cap;
        }
        return p;
    }
    // unmap every idle mapping (svt_trim): a long-lived embedding process gives the pool's memory back
    void trim()
    {
        std::vector<std::pair<void*, size_t>> idle;
        {
            std::lock_guard<std::mutex> g(lock_);
            idle.swap(idle_);
            idle_bytes_ = 0;
        }
        for (const auto& m : idle) munmap(m.first, m.second);
    }
    bool release_tracked(void* p)
    {
        size_t cap = 0;
        {
            std::lock_guard<std::mutex> g(lock_);
            auto it = lent_.find(p);
            if (it == lent_.end()) return false;
            cap = it->second;
            lent_.erase(it);
        }
        release(p, cap);
        return true;
    }

private:
    BufferPool()
    {
        if (const char* e = std::getenv("SVT_READER_POOL_MB")) limit_ = (size_t)std::max(0ll, std::atoll(e)) << 20;
    }
    static constexpr size_t kGrain = 2u << 20;           // one huge page
    std::mutex lock_;
    std::vector<std::pair<void*, size_t>> idle_;
    std::unordered_map<void*, size_t> lent_;
    size_t idle_bytes_ = 0, limit_ = (size_t)1024 << 20;
};

// append-only store of one worker: units are copied in whole, never split across chunks
class SummaryArena {
public:
    SummaryArena() = default;
    SummaryArena(const SummaryArena&) = delete;
    SummaryArena& operator=(const SummaryArena&) = delete;
    ~SummaryArena() { for (auto& c : chunks_) BufferPool::get().release(c.first, c.second); }
    const void* append(const void* data, size_t bytes)
    {
        if (bytes == 0) return nullptr;
        if (used_ + bytes > cap_) {
            size_t size = 0;     // 2, 4, 8, 16, 16 ... MiB: forty-seven workers of a small call do not map (and return) 16 MiB each
            void* p = BufferPool::get().acquire(std::max(bytes, std::min(kChunkBytes, (size_t)(2u << 20) << std::min<size_t>(chunks_.size(), 3))), &size);
            if (!p) return nullptr;
            chunks_.emplace_back(p, size);
            cap_ = size;
            used_ = 0;
        }
        uint8_t* dst = static_cast<uint8_t*>(chunks_.back().first) + used_;
        std::memcpy(dst, data, bytes);
        used_ += bytes;
        return dst;
    }

private:
    static constexpr size_t kChunkBytes = 16u << 20;
    std::vector<std::pair<void*, size_t>> chunks_;
    size_t cap_ = 0, used_ = 0;
};

inline double thread_cpu_seconds()
{
    timespec ts;
    return clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts) == 0 ? (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec : 0.0;
}

}  // namespace

// svt_trim()'s share of this file: the pooled huge-page buffers of the gather (up to SVT_READER_POOL_MB, 1 GiB by default)
extern "C" void svt_reads_trim() { BufferPool::get().trim(); }      // (internal: not in include/svtyper_reads.h)

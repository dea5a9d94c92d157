// svt_reads_handle.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): the BAM
// handle -- header + index (shared, read-only; file handles are per thread), the verify scope of a call -- and its entry points:
// open, close, accessors, the verify switch.  Needs: FileMap, Bgzf (svt_bgzf_reader.h).
#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC diagnostic ignored "-Wsubobject-linkage"   // (svt_bam is the C ABI's name; its FileMap is this translation unit's alone)
#endif
struct svt_bam {
    std::string path;
    FileMap file;
    std::string text;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lengths;
    std::unordered_map<std::string, int32_t> tid_of;
    uint64_t first_record = 0;
    svt::bamidx::Index index;      // BAI or CSI behind one model (svt_bam_index.h); kind KIND_NONE: the file has none
    bool has_index() const { return index.kind != svt::bamidx::KIND_NONE; }
    // CPU seconds per unit of the summariser's last calls on this file (0: none yet): sizes the next call's burst
    mutable std::atomic<double> cpu_s_per_unit{0.0};
    // svt_bam_set_verify: off by default; the tally of everything that was verified through this handle
    std::atomic<int> verify{0};
    mutable svt::VerifyTally tally;
};

static thread_local svt_bgzf_verify_counts g_verify_stats{};   // svt_bgzf_verify_stats: this thread's last call that took a handle

namespace svt {

VerifyTally* bam_verify(const svt_bam* bam) { return bam && bam->verify.load() ? &bam->tally : nullptr; }

VerifyScope::VerifyScope(const svt_bam* b) : bam(b)
{
    g_verify_stats = svt_bgzf_verify_counts{};
    if (!bam) return;
    verified = bam->tally.verified.load();
    failed = bam->tally.failed.load();
    host_ns = bam->tally.host_ns.load();
    device_ns = bam->tally.device_ns.load();
}
VerifyScope::~VerifyScope()
{
    if (!bam) return;
    g_verify_stats.members_verified = bam->tally.verified.load() - verified;
    g_verify_stats.members_failed = bam->tally.failed.load() - failed;
    g_verify_stats.host_crc_s = (double)(bam->tally.host_ns.load() - host_ns) * 1e-9;
    g_verify_stats.device_crc_s = (double)(bam->tally.device_ns.load() - device_ns) * 1e-9;
}

}  // namespace svt

extern "C" {

static int svt_bam_open_impl(const char* path, svt_bam** out)
{
    if (!path || !out) return fail(SVT_ERR_INVALID, "null argument");
    *out = nullptr;
    std::unique_ptr<svt_bam> b(new svt_bam());
    b->path = path;
    if (!b->file.open(b->path)) return fail(SVT_ERR_INVALID, std::string("cannot open ") + path);
    Bgzf z(b->file);
    if (!z.ok()) return fail(SVT_ERR_NOMEM, "cannot set up the inflate state");
    uint8_t magic[4];
    z.seek(0);
    auto rd32 = [&](int32_t& v) {
        uint8_t t[4];
        if (z.read(t, 4) != 4) return false;
        v = (int32_t)((uint32_t)t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24));
        return true;
    };
    int32_t l_text = 0, n_ref = 0;
    if (z.read(magic, 4) != 4 || std::memcmp(magic, "BAM\1", 4) != 0 || !rd32(l_text) || l_text < 0)
        return fail(SVT_ERR_INVALID, std::string(path) + " is not a BAM file");
    b->text.resize((size_t)l_text);
    if (l_text && z.read(&b->text[0], (size_t)l_text) != (size_t)l_text) return fail(SVT_ERR_INVALID, "truncated BAM header");
    b->text = b->text.c_str();   // cut at the first NUL
    if (!rd32(n_ref) || n_ref < 0) return fail(SVT_ERR_INVALID, "truncated BAM header");
    for (int32_t i = 0; i < n_ref; ++i) {
        int32_t l_name = 0, l_ref = 0;
        if (!rd32(l_name) || l_name <= 0) return fail(SVT_ERR_INVALID, "truncated BAM header");
        std::string name((size_t)l_name, '\0');
        if (z.read(&name[0], (size_t)l_name) != (size_t)l_name || !rd32(l_ref)) return fail(SVT_ERR_INVALID, "truncated BAM header");
        name.resize((size_t)l_name - 1);
        b->tid_of[name] = i;
        b->ref_names.push_back(name);
        b->ref_lengths.push_back(l_ref);
    }
    b->first_record = z.tell();
    // index: <path>.bai, the .bai next to the file, <path>.csi, the .csi next to it.  .bai first: a call that found its index
    // before this list grew reads the same file as before (htslib would take a .csi first; the answers are the same).  What a
    // file is, its magic says, not its name.
    std::string stem = b->path;
    const size_t dot = stem.rfind('.');
    if (dot != std::string::npos) stem = stem.substr(0, dot);
    const std::string cand[4] = {b->path + ".bai", stem + ".bai", b->path + ".csi", stem + ".csi"};
    for (const std::string& p : cand) {
        FILE* f = std::fopen(p.c_str(), "rb");
        if (!f) continue;
        std::vector<uint8_t> data;
        uint8_t tmp[65536];
        size_t n;
        while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) data.insert(data.end(), tmp, tmp + n);
        std::fclose(f);
        std::string err;
        if (!svt::bamidx::load(data.data(), data.size(), p, b->index, err)) return fail(SVT_ERR_INVALID, err);
        break;
    }
    if (!b->has_index()) return fail(SVT_ERR_INVALID, std::string("no .bai index found for ") + path + " (nor a .csi)");
    if (b->index.refs.size() < b->ref_names.size()) b->index.refs.resize(b->ref_names.size());
    *out = b.release();
    return SVT_OK;
}

int svt_bam_open(const char* path, svt_bam** out)
{
    return guarded([&] { return svt_bam_open_impl(path, out); });
}

void svt_bam_close(svt_bam* bam) { delete bam; }

int svt_bam_index_info(const svt_bam* bam, int* kind, int* min_shift, int* depth)
{
    if (!bam) return fail(SVT_ERR_INVALID, "null argument");
    if (kind) *kind = bam->index.kind;
    if (min_shift) *min_shift = bam->index.min_shift;
    if (depth) *depth = bam->index.depth;
    return SVT_OK;
}

int32_t svt_bam_n_references(const svt_bam* bam) { return bam ? (int32_t)bam->ref_names.size() : 0; }

const char* svt_bam_reference_name(const svt_bam* bam, int32_t tid)
{
    return (bam && tid >= 0 && tid < (int32_t)bam->ref_names.size()) ? bam->ref_names[tid].c_str() : nullptr;
}

int64_t svt_bam_reference_length(const svt_bam* bam, int32_t tid)
{
    return (bam && tid >= 0 && tid < (int32_t)bam->ref_lengths.size()) ? bam->ref_lengths[tid] : -1;
}

int32_t svt_bam_tid(const svt_bam* bam, const char* name)
{
    if (!bam || !name) return -1;
    auto it = bam->tid_of.find(name);
    return it == bam->tid_of.end() ? -1 : it->second;
}

const char* svt_bam_header_text(const svt_bam* bam) { return bam ? bam->text.c_str() : nullptr; }

int svt_bam_set_verify(svt_bam* bam, int on)
{
    return guarded([&]() -> int {
        if (!bam) return fail(SVT_ERR_INVALID, "null argument");
        bam->verify.store(on ? 1 : 0);
        return SVT_OK;
    });
}

int svt_bam_get_verify(const svt_bam* bam) { return bam ? bam->verify.load() : 0; }

int svt_bgzf_verify_stats(svt_bgzf_verify_counts* out)
{
    return guarded([&]() -> int {
        if (!out) return fail(SVT_ERR_INVALID, "null argument");
        *out = g_verify_stats;
        return SVT_OK;
    });
}

}  // extern "C"

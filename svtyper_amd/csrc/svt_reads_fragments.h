// svt_reads_fragments.h -- part of the translation unit svt_reads.cpp (included there, in order; not a stand-alone header): reads,
// pieces, fragments (what a record means is svt_record_rules.h): split-read QC, a unit's Workspace, process_unit, evidence_unit and
// a worker's UnitReader.  Needs: Bgzf, SharedBlocks (svt_bgzf_reader.h), svt_bam, bam_verify (svt_reads_handle.h), Record, fetch
// (svt_reads_records.h).
namespace {

struct ReadInfo {                // what a primary read contributes to a summary (svt_read_summary)
    int32_t tid = -1;
    int64_t start = 0, end = 0;
    bool reverse = false;
    int mapq = 0;
    int n_iv = 0;                // the (at most two) gap-free aligned intervals closest to the unit's breakends
    int64_t iv_start[2] = {0, 0}, iv_end[2] = {0, 0};
};

struct PieceOut {                // what a split piece contributes to a summary (svt_piece_summary)
    int32_t tid = 0;
    int64_t start = 0, end = 0, mapq = 0;
    bool reverse = false;
};

struct SplitOut {
    bool soft = false;
    PieceOut left, right;
};

struct Fragment {                // reused from unit to unit (its vectors keep their capacity)
    int lib = 0;
    int num_primary = 0;
    uint32_t name_off = 0, name_len = 0;   // query name in the workspace's name arena
    std::vector<uint16_t> seen;            // flags already added under this query name (parsers.py:748-754)
    std::vector<ReadInfo> primaries;
    std::vector<SplitOut> splits;
    void reset(int library, uint32_t off, uint32_t len)
    {
        lib = library;
        num_primary = 0;
        name_off = off;
        name_len = len;
        seen.clear();
        primaries.clear();
        splits.clear();
    }
};

// SplitRead.is_valid (parsers.py:959-1058 / fragments.py) -> fills `out` when the candidate is valid
// returns 1 valid, 0 invalid, -1 malformed input.  The rules are rr::; the host reader's own: an SA number is what strtoll
// reads over the whole field, a chromosome name goes through the header's map, and there is no limit on lengths.
int split_candidate(const svt_bam& bam, const Record& r, const rr::Tags& t, SplitOut& out)
{
    if (r.n_cigar == 0) return 0;   // a mapped read without a CIGAR cannot be a split candidate (fragments.py: add_read)
    rr::CigarStats a;
    rr::cigar_of_words(r.cigar(), r.n_cigar, a);
    const bool a_rev = (r.flag & 0x10) != 0;
    const PieceOut self{r.tid, r.pos, r.end, (int64_t)r.mapq, a_rev};
    bool self_left;
    PieceOut other;
    if (!t.have_sa) {
        if (!rr::soft_clip_candidate(a, r.l_seq)) return 0;
        other = PieceOut{-2, 1, 1, 0, a_rev};           // the dummy piece (chrom None)
        self_left = !rr::left_clipped(a);
    } else {
        const uint8_t* sa = r.data + t.sa_off;
        uint32_t fo[5], fl[5];
        uint32_t entries;
        const uint32_t fields = rr::sa_fields(sa, t.sa_len, entries, fo, fl);
        if (entries > 1) return 0;                      // more than one entry -> discarded (:992-993)
        if (fields < 5) return -1;
        auto whole_number = [&](int k, long long& v) {  // strtoll over the whole field
            char buf[32];
            if (fl[k] == 0 || fl[k] >= sizeof buf) return false;
            std::memcpy(buf, sa + fo[k], fl[k]);
            buf[fl[k]] = 0;
            char* endp = nullptr;
            v = std::strtoll(buf, &endp, 10);
            return *endp == 0;
        };
        long long mate_pos1 = 0, mate_mapq = 0;
        rr::CigarStats b;
        if (!whole_number(1, mate_pos1) || !whole_number(4, mate_mapq)) return -1;
        if (rr::cigar_of_string(sa + fo[3], fl[3], UINT32_MAX, 18, b) != rr::CIGAR_OK) return -1;
        const std::string sa_chrom(reinterpret_cast<const char*>(sa) + fo[0], fl[0]);    // (chromosome names fit the small-string buffer)
        auto it = bam.tid_of.find(sa_chrom);
        const bool b_rev = fl[2] == 1 && sa[fo[2]] == '-';
        other = PieceOut{it == bam.tid_of.end() ? -3 : it->second, mate_pos1 - 1, mate_pos1 - 1 + b.ref, mate_mapq, b_rev};
        const rr::Piece pa = {self.tid, self.start, self.end, a_rev, rr::query_pos(a, a_rev)};
        const rr::Piece pb = {other.tid, other.start, other.end, b_rev, rr::query_pos(b, b_rev)};
        const bool same_chrom = r.tid >= 0 && bam.ref_names[r.tid] == sa_chrom;
        if (!rr::split_valid(pa, pb, same_chrom, rr::left_clipped(a), self_left)) return 0;
    }
    out.soft = !t.have_sa;
    out.left = self_left ? self : other;
    out.right = self_left ? other : self;
    return 1;
}

void fill_read(svt_read_summary& d, const ReadInfo& r)
{
    d.tid = r.tid;
    d.start = clip32(r.start);
    d.end = clip32(r.end);
    for (int k = 0; k < r.n_iv; ++k) {
        d.iv_start[k] = clip32(r.iv_start[k]);
        d.iv_end[k] = clip32(r.iv_end[k]);
    }
    d.mapq = (uint8_t)r.mapq;
    d.flags = (uint8_t)(SVT_READ_PRESENT | (r.reverse ? SVT_READ_REVERSE : 0));
}

bool fill_piece(svt_piece_summary& d, const PieceOut& p)
{
    if (p.mapq < 0) return false;
    d.tid = p.tid;
    d.start = clip32(p.start);
    d.end = clip32(p.end);
    d.mapq = (uint8_t)std::min<int64_t>(p.mapq, 255);   // an SA-tag MAPQ above 255: prob_mapq is exactly 1.0 from 163 on (packer.py: _mapq)
    d.flags = (uint8_t)(SVT_READ_PRESENT | (p.reverse ? SVT_READ_REVERSE : 0));
    return true;
}

struct UnitOut {                       // per worker, reused for every unit it processes
    std::vector<svt_fragment> frags;
    std::vector<svt_record> recs;      // svt_bam_evidence: the summaries turned into evidence records
    bool skipped = false;
};

// Per-worker scratch of process_unit, reused from unit to unit so that a read costs no allocation: the
// read-fragments of the unit (query name -> Fragment) live in a vector indexed through an open-addressing
// hash table over a name arena, and are emitted in sorted(query_name) order at the end.
struct Workspace {
    std::vector<Fragment> frags;       // [0, n_frags) are live
    size_t n_frags = 0;
    std::vector<char> names;
    std::vector<uint64_t> table;       // (name hash's high half) << 32 | fragment index + 1, 0 = empty; size is a power of two
    std::vector<uint32_t> order;
    std::vector<std::pair<uint64_t, uint32_t>> keys;
    std::vector<uint64_t> packed;
    std::vector<const SplitOut*> seq, clip;
    std::string last_rg;               // most reads of a unit share their read group
    int32_t last_lib = 0;
    bool have_last_rg = false;

    void begin_unit()
    {
        n_frags = 0;
        names.clear();
        if (table.size() < 1024) table.assign(1024, 0ull);
        else std::fill(table.begin(), table.end(), 0ull);
    }
    static uint64_t hash_name(const char* p, size_t n)
    {
        // eight bytes per step: a byte-wise FNV-1a is a serial chain of one multiply per byte of a 20-50 byte name (a tenth of
        // what a kept read costs)
        uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
        size_t i = 0;
        for (; i + 8 <= n; i += 8) {
            uint64_t w;
            std::memcpy(&w, p + i, 8);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        if (i < n) {
            uint64_t w = 0;
            std::memcpy(&w, p + i, n - i);
            h = (h ^ w) * 0xFF51AFD7ED558CCDull;
            h ^= h >> 32;
        }
        return h;
    }
    const char* name_of(const Fragment& f) const { return names.data() + f.name_off; }
    // the fragment of this query name; created (with `lib`) when the name is new
    Fragment& fragment(const char* name, const uint32_t len, int lib)
    {
        if ((n_frags + 1) * 2 > table.size()) grow();
        const size_t mask = table.size() - 1;
        const uint64_t h = hash_name(name, len), tag = h & 0xffffffff00000000ull;
        // the slot carries the hash's high half: a probe that meets another name's slot moves on without touching that
        // fragment (a big struct) or its name; the second read of a pair pays ONE memcmp
        for (size_t i = h & mask;; i = (i + 1) & mask) {
            const uint64_t e = table[i];
            if (e == 0ull) {
                if (n_frags == frags.size()) frags.emplace_back();
                Fragment& f = frags[n_frags];
                f.reset(lib, (uint32_t)names.size(), len);
                names.insert(names.end(), name, name + len);
                table[i] = tag | (uint64_t)++n_frags;
                return f;
            }
            if ((e & 0xffffffff00000000ull) != tag) continue;
            Fragment& f = frags[(uint32_t)e - 1];
            if (f.name_len == len && std::memcmp(name_of(f), name, len) == 0) return f;
        }
    }
    void grow()
    {
        table.assign(table.size() * 2, 0ull);
        const size_t mask = table.size() - 1;
        for (size_t k = 0; k < n_frags; ++k) {
            const uint64_t h = hash_name(name_of(frags[k]), frags[k].name_len);
            size_t i = h & mask;
            while (table[i]) i = (i + 1) & mask;
            table[i] = (h & 0xffffffff00000000ull) | (uint64_t)(k + 1);
        }
    }
    // live fragments in the order of Python's sorted() over their (ASCII) names.  Query names of one run share a long
    // prefix (instrument : run : flowcell : lane ...), so comparing them byte by byte from the start -- a few hundred
    // times per unit -- reads the same thirty bytes again and again: the common prefix of the unit's names is found once
    // and the sort runs on the eight bytes behind it as one big-endian integer; equal keys fall back to the whole names.
    const std::vector<uint32_t>& sorted_order()
    {
        order.resize(n_frags);
        keys.resize(n_frags);
        size_t lcp = n_frags ? frags[0].name_len : 0;
        for (size_t k = 1; k < n_frags && lcp; ++k) {
            const char *a = name_of(frags[0]), *b = name_of(frags[k]);
            const size_t n = std::min<size_t>(lcp, frags[k].name_len);
            size_t i = 0;
            for (; i + 8 <= n; i += 8) {      // eight bytes at a time: thirty common bytes times a few hundred names per unit
                uint64_t x, y;
                std::memcpy(&x, a + i, 8);
                std::memcpy(&y, b + i, 8);
                if (x != y) { i += (size_t)__builtin_ctzll(x ^ y) >> 3; break; }     // (little-endian: the lowest differing byte)
            }
            while (i < n && a[i] == b[i]) ++i;      // (the tail; at once over when the words differed)
            lcp = i;
        }
        auto key_of = [&](const Fragment& f) {
            uint64_t key = 0;                                    // bytes past the end count as 0: a shorter name sorts first,
            const unsigned char* p = reinterpret_cast<const unsigned char*>(name_of(f)) + lcp;   // as it does for memcmp + length
            const size_t have = f.name_len - lcp;               // (lcp <= every name's length)
            if (have >= 8) {
                std::memcpy(&key, p, 8);
                return __builtin_bswap64(key);
            }
            for (size_t i = 0; i < 8; ++i) key = (key << 8) | (i < have ? p[i] : 0u);
            return key;
        };
        auto by_name = [&](const uint32_t x, const uint32_t y) {
            const Fragment &a = frags[x], &b = frags[y];
            const int c = std::memcmp(name_of(a), name_of(b), std::min(a.name_len, b.name_len));
            return c != 0 ? c < 0 : a.name_len < b.name_len;
        };
        if (n_frags <= 4096) {
            // the usual unit: the key's leading 52 bits and the fragment's index in ONE integer -- a sort of plain 64-bit words, no
            // comparator that looks at the names; runs of equal leading bits (rare: they agree in six and a half bytes behind the
            // common prefix) are put in order by their whole names afterwards
            packed.resize(n_frags);
            for (size_t k = 0; k < n_frags; ++k) packed[k] = (key_of(frags[k]) & ~uint64_t(0xfff)) | (uint64_t)k;
            std::sort(packed.begin(), packed.end());
            for (size_t k = 0; k < n_frags; ++k) order[k] = (uint32_t)(packed[k] & 0xfffu);
            for (size_t k = 0; k < n_frags;) {
                size_t e = k + 1;
                while (e < n_frags && (packed[e] >> 12) == (packed[k] >> 12)) ++e;
                if (e - k > 1) std::sort(order.begin() + (ptrdiff_t)k, order.begin() + (ptrdiff_t)e, by_name);
                k = e;
            }
            return order;
        }
        for (size_t k = 0; k < n_frags; ++k) keys[k] = std::make_pair(key_of(frags[k]), (uint32_t)k);
        std::sort(keys.begin(), keys.end(), [&](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) {
            if (x.first != y.first) return x.first < y.first;
            return by_name(x.second, y.second);
        });
        for (size_t k = 0; k < n_frags; ++k) order[k] = keys[k].second;
        return order;
    }
};

// one unit: gather reads of both windows, assemble fragments, emit summaries
// `emit(fragment)`: what becomes of a finished summary -- kept as it is (svt_bam_summarise) or turned into its 16-byte evidence
// record on the spot (svt_bam_evidence: no array of 128-byte summaries in between); returns false with `err` set to stop
template <typename Emit>
int process_unit(const svt_bam& bam, Bgzf& z, std::vector<uint8_t>& buf, const svt_summarise_args& A,
                 const std::unordered_map<std::string, int32_t>& rg_lib, uint64_t u, Workspace& ws, UnitOut& out,
                 std::string& err, Emit&& emit)
{
    out.frags.clear();
    out.recs.clear();
    out.skipped = false;
    const svt_fetch_unit& w = A.windows[u];
    const int32_t tids[2] = {w.tid_a, w.tid_b};
    const int64_t los[2] = {w.lo_a, w.lo_b}, his[2] = {w.hi_a, w.hi_b};
    const int64_t near_a = A.breakpoints[u].pos_a, near_b = A.breakpoints[u].pos_b;
    ws.begin_unit();
    int rc = SVT_OK;

    // count_mode 1 (singlesample.py:158-185): a unit is skipped when bam.count() of either window exceeds
    // max_reads.  count() looks at the same records the gather pass walks, so the two are one pass here: the
    // reads of a window are counted (pysam's filter: not unmapped / secondary / QC-fail / duplicate) while
    // they are gathered, and the unit is dropped when a window turns out to be over the limit.
    const bool count_windows = A.count_mode == 1 && A.max_reads >= 0;
    for (int s = 0; s < 2 && !out.skipped; ++s) {
        int64_t i = -1, n_counted = 0;
        const bool ok = fetch(bam, z, tids[s], los[s], his[s], buf, [&](const Record& r) {
            ++i;                                                        // enumerate() index of classic.py:79
            if (count_windows && !(r.flag & (0x4 | 0x100 | 0x200 | 0x400)) && ++n_counted > A.max_reads) {
                out.skipped = true;
                return false;
            }
            if (r.flag & (0x4 | 0x400)) return true;                   // unmapped / duplicate
            rr::Tags tags;
            uint32_t behind_rg = 0;
            const char* rg = read_group(r, tags, behind_rg);
            if (!rg) { err = "read without a usable RG tag: " + r.name_str(); rc = SVT_ERR_INVALID; return false; }
            if (!ws.have_last_rg || ws.last_rg != rg) {
                auto it = rg_lib.find(rg);
                if (it == rg_lib.end()) { err = std::string("read group not in the library table: ") + rg; rc = SVT_ERR_INVALID; return false; }
                ws.last_rg = rg;
                ws.last_lib = it->second;
                ws.have_last_rg = true;
            }
            if (ws.last_lib < 0) return true;                           // library below the prevalence cut
            if (A.count_mode == 0 && A.max_reads >= 0 && i > A.max_reads) { out.skipped = true; return false; }
            Fragment& f = ws.fragment(r.name(), r.name_len(), ws.last_lib);             // SamFragment(read, lib) when new
            if (std::find(f.seen.begin(), f.seen.end(), r.flag) != f.seen.end()) return true;   // same (name, flag) again
            f.seen.push_back(r.flag);
            if (r.flag & (0x100 | 0x800)) return true;                  // secondary / supplementary
            ReadInfo ri;
            ri.tid = r.tid;
            ri.start = r.pos;
            ri.end = r.end;
            ri.reverse = (r.flag & 0x10) != 0;
            ri.mapq = (int)r.mapq;
            rr::Intervals iv;
            rr::aligned_intervals(r.cigar(), r.n_cigar, r.pos, near_a, near_b, iv);
            ri.n_iv = (int)iv.n;
            for (int k = 0; k < 2; ++k) { ri.iv_start[k] = iv.s[k]; ri.iv_end[k] = iv.e[k]; }
            f.primaries.push_back(ri);
            f.num_primary += 1;
            SplitOut sp;
            const int v = tags_behind_rg(r, tags, behind_rg) ? split_candidate(bam, r, tags, sp) : -1;
            if (v < 0) { err = "malformed SA tag / CIGAR at read " + r.name_str(); rc = SVT_ERR_INVALID; return false; }
            if (v > 0) f.splits.push_back(sp);
            return true;
        });
        if (rc != SVT_OK) return rc;
        if (!ok) { err = z.crc_failed() ? z.crc_error() : "BAM read error"; return SVT_ERR_INVALID; }
    }
    if (out.skipped) { out.frags.clear(); out.recs.clear(); return SVT_OK; }

    for (const uint32_t fi : ws.sorted_order()) {
        const Fragment& f = ws.frags[fi];
        ws.seq.clear();
        ws.clip.clear();
        for (const SplitOut& sp : f.splits) (sp.soft ? ws.clip : ws.seq).push_back(&sp);
        const size_t n_rec = std::max<size_t>({(size_t)1, (f.primaries.size() + 1) / 2, ws.seq.size(), ws.clip.size()});
        for (size_t k = 0; k < n_rec; ++k) {
            svt_fragment fr;
            std::memset(&fr, 0, sizeof fr);
            fr.read[0].tid = fr.read[1].tid = -1;
            for (int j = 0; j < 2; ++j)
                if (2 * k + j < f.primaries.size()) fill_read(fr.read[j], f.primaries[2 * k + j]);
            fr.read[0].reserved = (uint16_t)f.lib;
            fr.read[1].reserved = (uint16_t)(((k == 0 && f.num_primary == 2) ? SVT_FRAG_PAIR : 0) | (k > 0 ? SVT_FRAG_CONTINUATION : 0));
            bool ok = true;
            if (k < ws.seq.size()) ok = fill_piece(fr.seq[0], ws.seq[k]->left) && fill_piece(fr.seq[1], ws.seq[k]->right);
            if (ok && k < ws.clip.size()) ok = fill_piece(fr.clip[0], ws.clip[k]->left) && fill_piece(fr.clip[1], ws.clip[k]->right);
            if (!ok) {
                err = "MAPQ outside 0..255 in an SA tag of fragment " + std::string(ws.name_of(f), f.name_len);
                return SVT_ERR_INVALID;
            }
            if (!emit(fr)) return SVT_ERR_INVALID;
        }
    }
    return SVT_OK;
}

// one unit as evidence records (unit.recs): process_unit with the predicates of the device stage as its emitter
int evidence_unit(const svt_bam& bam, Bgzf& z, std::vector<uint8_t>& buf, const svt_summarise_args& A, const svt_evidence_params& G,
                  const std::unordered_map<std::string, int32_t>& rg_lib, uint64_t u, Workspace& ws, UnitOut& unit, std::string& err)
{
    const svt_breakpoint& bp = A.breakpoints[u];
    if (bp.svtype > SVT_SVTYPE_BND) { err = "bad svtype"; return SVT_ERR_INVALID; }
    return process_unit(bam, z, buf, A, rg_lib, u, ws, unit, err, [&](const svt_fragment& f) {
        const uint32_t lib = f.read[0].reserved;
        if (lib >= G.n_libs) { err = "library index of a fragment outside the library table"; return false; }
        const svt::Record4 r = svt::geometry_record(svt::read_of(f.read[0]), svt::read_of(f.read[1]), svt::piece_of(f.seq[0]),
                                                    svt::piece_of(f.seq[1]), svt::piece_of(f.clip[0]), svt::piece_of(f.clip[1]), bp,
                                                    G.lib_flank[lib], G.min_aligned, G.split_slop);
        static_assert(sizeof(svt_record) == sizeof r, "svt_record is four words");
        unit.recs.emplace_back();
        std::memcpy(&unit.recs.back(), &r, sizeof r);
        return true;
    });
}

using RgLibraries = std::unordered_map<std::string, int32_t>;         // read group -> library index (below 0: under the prevalence cut)
RgLibraries rg_library_map(const svt_summarise_args& A)
{
    RgLibraries rg_lib;
    for (uint32_t i = 0; i < A.n_read_groups; ++i) rg_lib[A.read_groups[i]] = A.read_group_lib[i];
    return rg_lib;
}

// What one worker thread reads units with, reused from unit to unit; `unit` holds the one read last.  geometry: for evidence().
struct UnitReader {
    const svt_bam& bam;
    const svt_summarise_args& A;
    const svt_evidence_params* geometry;
    const RgLibraries& rg_lib;
    Bgzf z;
    std::vector<uint8_t> buf;
    UnitOut unit;
    Workspace ws;
    UnitReader(const svt_bam* b, const svt_summarise_args* a, const svt_evidence_params* g, const RgLibraries& m, SharedBlocks* shared) : bam(*b), A(*a), geometry(g), rg_lib(m), z(b->file, shared, svt::bam_verify(b)) {}
    bool ok() const { return z.ok(); }
    int evidence(uint64_t u, std::string& err) { return evidence_unit(bam, z, buf, A, *geometry, rg_lib, u, ws, unit, err); }
    int summaries(uint64_t u, std::string& err) { return process_unit(bam, z, buf, A, rg_lib, u, ws, unit, err, [&](const svt_fragment& f) { unit.frags.push_back(f); return true; }); }
};

}  // namespace

// svt_cram.h -- one CRAM 3.0 slice as BAM records (CRAM format specification 3.0, sections 8 to 12): host C++, no HIP.
//
// In: the slice's blocks as they are once their block method is undone (the core block and the external blocks with their
// content ids), the content of the container's compression header block and of the slice header block, the @RG ids of the SAM
// header in order.  Out: the slice's records as BAM record bytes, block_size first, side by side, with a table of offsets -- what
// AlignedSegment, record_of, RecordSink and the sorted `-w` writer take from a BAM.
//
// What SVTyper reads of a record is its name, flag, positions, MAPQ, CIGAR, mate fields, TLEN and tags; all of these follow from
// the record's data series and read features without the reference sequence.  Bases and qualities are NOT reconstructed: SEQ is
// written as `N` x RL and QUAL as 0xFF x RL (a record stored without its sequence, CF bit 8, has none here either: l_seq 0), `bin` is reg2bin of the record's extent.  Every series a record uses is still read
// through its codec (BA, QS, BS, IN, SC, BB, QQ), so that blocks several series share stay in step.
//
// CIGAR from the read features: the read bases between features are M; X, B and b are M too; I and i are I; D, N, S, H and P are
// themselves; q and Q add nothing; neighbours of one kind are merged; an unmapped read has none.
//
// Mates.  A detached record (CF bit 2) takes MF, NS, NP and TS as stored.  Records attached by NF (CF bit 4) form a chain inside
// the slice: a record's mate is the next of its chain, the last one's the first; next reference, next position and the flags
// 0x20 and 0x8 come from that mate; TLEN is the chain's rightmost aligned end minus its leftmost aligned start plus 1 (0 when
// one of them is unmapped or they lie on several references), positive for the record that starts leftmost -- at equal starts
// the earliest in the slice -- and negative for the others.  That tie rule is this project's reading of the format's text.
// Without preserved names the records of a chain are all named by the record counter of its first.
//
// Encodings: NULL, EXTERNAL, HUFFMAN (with the code of no bits for one symbol), BYTE_ARRAY_LEN, BYTE_ARRAY_STOP, BETA, SUBEXP,
// GAMMA.  GOLOMB and GOLOMB_RICE are refused.  Every read is checked against the end of its block: a slice that reads past one is
// refused (Refuse), nothing is repaired.
#ifndef SVT_CRAM_H
#define SVT_CRAM_H

#include <stdint.h>

#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace svt {
namespace cram {

struct Refuse : std::runtime_error {
    explicit Refuse(const std::string& what) : std::runtime_error(what) {}
};

// bytes read in order: a block, or a part of one
struct Bytes {
    const uint8_t* p = nullptr;
    size_t n = 0, at = 0;
    std::string name;
    [[noreturn]] void past() const { throw Refuse(name + ": an encoding reads past its block"); }
    uint8_t u8()
    {
        if (at >= n) past();
        return p[at++];
    }
    const uint8_t* take(size_t k)
    {
        if (k > n - at) past();
        const uint8_t* q = p + at;
        at += k;
        return q;
    }
    int32_t itf8()
    {
        const uint32_t b = u8();
        if (b < 0x80) return (int32_t)b;
        if (b < 0xC0) return (int32_t)(((b & 0x3F) << 8) | u8());
        if (b < 0xE0) {
            const uint32_t b1 = u8(), b2 = u8();
            return (int32_t)(((b & 0x1F) << 16) | (b1 << 8) | b2);
        }
        if (b < 0xF0) {
            const uint32_t b1 = u8(), b2 = u8(), b3 = u8();
            return (int32_t)(((b & 0x0F) << 24) | (b1 << 16) | (b2 << 8) | b3);
        }
        const uint32_t b1 = u8(), b2 = u8(), b3 = u8(), b4 = u8();
        return (int32_t)(((b & 0x0F) << 28) | (b1 << 20) | (b2 << 12) | (b3 << 4) | (b4 & 0x0F));
    }
    int64_t ltf8()
    {
        const uint32_t b = u8();
        uint32_t extra = 0;
        while (extra < 8 && (b & (0x80u >> extra))) ++extra;
        uint64_t v = extra < 7 ? (b & (0xFFu >> (extra + 1))) : 0;
        for (uint32_t i = 0; i < extra; ++i) v = (v << 8) | u8();
        return (int64_t)v;
    }
};

// the core block, bit by bit from each byte's top
struct Bits {
    const uint8_t* p = nullptr;
    size_t n = 0, bit = 0;
    uint32_t get(uint32_t k)
    {
        if (k > 32) throw Refuse("core block: a code of more than 32 bits");
        uint32_t v = 0;
        for (uint32_t i = 0; i < k; ++i) {
            if ((bit >> 3) >= n) throw Refuse("core block: an encoding reads past its block");
            v = (v << 1) | ((p[bit >> 3] >> (7 - (bit & 7))) & 1u);
            ++bit;
        }
        return v;
    }
};

enum Kind : int32_t { E_NULL = 0, E_EXTERNAL = 1, E_GOLOMB = 2, E_HUFFMAN = 3, E_BYTE_ARRAY_LEN = 4, E_BYTE_ARRAY_STOP = 5, E_BETA = 6, E_SUBEXP = 7,
                      E_GOLOMB_RICE = 8, E_GAMMA = 9 };

struct Codec {
    int32_t kind = -1;                  // -1: the compression header has no encoding for the series
    std::string series;
    int32_t content_id = 0, offset = 0, bits = 0;
    uint8_t stop = 0;
    Bytes* ext = nullptr;               // (EXTERNAL, BYTE_ARRAY_STOP) the slice's block of content_id; null: there is none
    struct Code { int32_t len; uint32_t code; int32_t sym; };
    std::vector<Code> huff;             // by length, then by code
    std::unique_ptr<Codec> len_codec, val_codec;
};

inline void parse_codec(Bytes& in, Codec& c, const std::string& series)
{
    c.series = series;
    c.kind = in.itf8();
    const int32_t size = in.itf8();
    if (size < 0) throw Refuse(series + ": an encoding of negative size");
    Bytes par;
    par.p = in.take((size_t)size);
    par.n = (size_t)size;
    par.name = "compression header (" + series + ")";
    switch (c.kind) {
    case E_NULL: break;
    case E_EXTERNAL: c.content_id = par.itf8(); break;
    case E_GOLOMB: throw Refuse(series + ": the GOLOMB encoding (2) is not read");
    case E_GOLOMB_RICE: throw Refuse(series + ": the GOLOMB_RICE encoding (8) is not read");
    case E_HUFFMAN: {
        const int32_t n = par.itf8();
        if (n < 0 || (size_t)n > par.n) throw Refuse(series + ": HUFFMAN alphabet size");
        std::vector<int32_t> syms((size_t)n);
        for (auto& s : syms) s = par.itf8();
        const int32_t m = par.itf8();
        if (m != n) throw Refuse(series + ": HUFFMAN alphabet and bit lengths differ in number");
        c.huff.resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
            const int32_t len = par.itf8();
            if (len < 0 || len > 31) throw Refuse(series + ": HUFFMAN bit length");
            c.huff[i] = Codec::Code{len, 0, syms[i]};
        }
        for (size_t i = 1; i < c.huff.size(); ++i)             // (alphabets are small: insertion sort by length, then symbol)
            for (size_t j = i; j > 0 && (c.huff[j].len < c.huff[j - 1].len || (c.huff[j].len == c.huff[j - 1].len && c.huff[j].sym < c.huff[j - 1].sym)); --j)
                std::swap(c.huff[j], c.huff[j - 1]);
        uint32_t code = 0;
        int32_t len = c.huff.empty() ? 0 : c.huff[0].len;
        for (auto& h : c.huff) {
            code <<= (h.len - len);
            len = h.len;
            h.code = code++;
        }
        break;
    }
    case E_BYTE_ARRAY_LEN:
        c.len_codec.reset(new Codec());
        c.val_codec.reset(new Codec());
        parse_codec(par, *c.len_codec, series + " lengths");
        parse_codec(par, *c.val_codec, series + " values");
        break;
    case E_BYTE_ARRAY_STOP:
        c.stop = par.u8();
        c.content_id = par.itf8();
        break;
    case E_BETA:
        c.offset = par.itf8();
        c.bits = par.itf8();
        if (c.bits < 0 || c.bits > 32) throw Refuse(series + ": BETA bit count");
        break;
    case E_SUBEXP:
        c.offset = par.itf8();
        c.bits = par.itf8();
        if (c.bits < 0 || c.bits > 31) throw Refuse(series + ": SUBEXP k");
        break;
    case E_GAMMA: c.offset = par.itf8(); break;
    default: throw Refuse(series + ": unknown encoding " + std::to_string(c.kind));
    }
}

// the compression header of a container
struct Header {
    bool names = true, ap_delta = true;
    std::vector<std::vector<uint32_t>> tag_lists;           // TD: per entry the tag ids (c1 << 16 | c2 << 8 | type)
    std::map<std::string, Codec> series;
    std::map<uint32_t, Codec> tags;
};

inline void parse_header(const uint8_t* p, size_t n, Header& h)
{
    Bytes in;
    in.p = p;
    in.n = n;
    in.name = "compression header";
    {   // preservation map
        const int32_t size = in.itf8();
        if (size < 0) throw Refuse("compression header: preservation map size");
        Bytes m;
        m.p = in.take((size_t)size);
        m.n = (size_t)size;
        m.name = "preservation map";
        const int32_t count = m.itf8();
        for (int32_t i = 0; i < count; ++i) {
            const uint8_t a = m.u8(), b = m.u8();
            const std::string key{(char)a, (char)b};
            if (key == "RN") h.names = m.u8() != 0;
            else if (key == "AP") h.ap_delta = m.u8() != 0;
            else if (key == "RR") (void)m.u8();
            else if (key == "SM") (void)m.take(5);
            else if (key == "TD") {
                const int32_t len = m.itf8();
                if (len < 0) throw Refuse("preservation map: TD size");
                const uint8_t* td = m.take((size_t)len);
                std::vector<uint32_t> cur;
                size_t at = 0;
                while (at < (size_t)len) {
                    if (td[at] == 0) {
                        h.tag_lists.push_back(cur);
                        cur.clear();
                        ++at;
                        continue;
                    }
                    if ((size_t)len - at < 3) throw Refuse("preservation map: a TD entry of less than three bytes");
                    cur.push_back((uint32_t)td[at] << 16 | (uint32_t)td[at + 1] << 8 | td[at + 2]);
                    at += 3;
                }
                if (!cur.empty()) h.tag_lists.push_back(cur);
            } else {
                throw Refuse("preservation map: unknown key " + key);
            }
        }
    }
    {   // data series
        const int32_t size = in.itf8();
        if (size < 0) throw Refuse("compression header: data series map size");
        Bytes m;
        m.p = in.take((size_t)size);
        m.n = (size_t)size;
        m.name = "data series map";
        const int32_t count = m.itf8();
        for (int32_t i = 0; i < count; ++i) {
            const uint8_t a = m.u8(), b = m.u8();
            const std::string key{(char)a, (char)b};
            parse_codec(m, h.series[key], key);
        }
    }
    {   // tags
        const int32_t size = in.itf8();
        if (size < 0) throw Refuse("compression header: tag map size");
        Bytes m;
        m.p = in.take((size_t)size);
        m.n = (size_t)size;
        m.name = "tag map";
        const int32_t count = m.itf8();
        for (int32_t i = 0; i < count; ++i) {
            const uint32_t key = (uint32_t)m.itf8();
            const std::string name{(char)(key >> 16), (char)(key >> 8), ':', (char)key};
            parse_codec(m, h.tags[key], "tag " + name);
        }
    }
}

// one slice being decoded: its blocks, where each is read, the codecs bound to them
struct Slice {
    Bits core;
    std::map<int32_t, Bytes> ext;

    void bind(Codec& c)
    {
        if (c.kind == E_EXTERNAL || c.kind == E_BYTE_ARRAY_STOP) {
            auto it = ext.find(c.content_id);
            c.ext = it == ext.end() ? nullptr : &it->second;
        }
        if (c.len_codec) bind(*c.len_codec);
        if (c.val_codec) bind(*c.val_codec);
    }
    Bytes& block(const Codec& c)
    {
        if (!c.ext) throw Refuse(c.series + ": the slice has no block of content id " + std::to_string(c.content_id));
        return *c.ext;
    }
    // an integer (as_byte: a value of a byte series, which EXTERNAL stores as one byte)
    int32_t value(Codec& c, bool as_byte)
    {
        switch (c.kind) {
        case -1: throw Refuse(c.series + ": a record uses the series and the compression header has no encoding for it");
        case E_NULL: return 0;
        case E_EXTERNAL: return as_byte ? (int32_t)block(c).u8() : block(c).itf8();
        case E_HUFFMAN: {
            uint32_t code = 0;
            int32_t len = 0;
            for (const auto& h : c.huff) {
                if (h.len > len) {
                    code = (code << (h.len - len)) | core.get((uint32_t)(h.len - len));
                    len = h.len;
                }
                if (h.code == code) return h.sym;
            }
            throw Refuse(c.series + ": a HUFFMAN code of no symbol");
        }
        case E_BETA: return (int32_t)(core.get((uint32_t)c.bits) - (uint32_t)c.offset);
        case E_GAMMA: {
            uint32_t zeros = 0;
            while (core.get(1) == 0)
                if (++zeros > 31) throw Refuse(c.series + ": a GAMMA code of more than 32 bits");
            return (int32_t)(((1u << zeros) | core.get(zeros)) - (uint32_t)c.offset);
        }
        case E_SUBEXP: {
            uint32_t ones = 0;
            while (core.get(1) == 1)
                if (++ones > 32) throw Refuse(c.series + ": a SUBEXP code of more than 32 ones");
            uint32_t v;
            if (ones == 0) {
                v = core.get((uint32_t)c.bits);
            } else {
                const uint32_t b = ones + (uint32_t)c.bits - 1;
                if (b > 31) throw Refuse(c.series + ": a SUBEXP code of more than 32 bits");
                v = (1u << b) | core.get(b);
            }
            return (int32_t)(v - (uint32_t)c.offset);
        }
        default: throw Refuse(c.series + ": the encoding " + std::to_string(c.kind) + " holds no single value");
        }
    }
    // a byte array, appended to *out (null: read and dropped).  -> its length
    size_t array(Codec& c, std::vector<uint8_t>* out)
    {
        switch (c.kind) {
        case -1: throw Refuse(c.series + ": a record uses the series and the compression header has no encoding for it");
        case E_NULL: return 0;
        case E_BYTE_ARRAY_STOP: {
            Bytes& b = block(c);
            const size_t from = b.at;
            while (b.u8() != c.stop) {}
            if (out) out->insert(out->end(), b.p + from, b.p + b.at - 1);
            return b.at - 1 - from;
        }
        case E_BYTE_ARRAY_LEN: {
            const int32_t len = value(*c.len_codec, false);
            if (len < 0) throw Refuse(c.series + ": a byte array of negative length");
            Codec& v = *c.val_codec;
            if (v.kind == E_EXTERNAL) {
                const uint8_t* p = block(v).take((size_t)len);
                if (out) out->insert(out->end(), p, p + len);
            } else {
                for (int32_t i = 0; i < len; ++i) {
                    const uint8_t x = (uint8_t)value(v, true);
                    if (out) out->push_back(x);
                }
            }
            return (size_t)len;
        }
        default: throw Refuse(c.series + ": the encoding " + std::to_string(c.kind) + " holds no byte array");
        }
    }
};

struct Rec {
    int32_t flag = 0, cf = 0, ref = -1, rl = 0, pos = -1, rg = -1, mapq = 0, next_ref = -1, next_pos = -1, tlen = 0, nf = -1;
    int64_t end = 0;                    // behind the last aligned reference base (pos + 1 without a CIGAR)
    int64_t next = -1, head = -1;       // (attached) the next record of the chain; the chain's first
    std::string name;
    std::vector<uint32_t> cigar;        // BAM: len << 4 | op
    std::vector<uint8_t> aux;
};

inline void add_op(Rec& r, uint32_t op, int64_t len)
{
    if (len <= 0) return;
    if (len >= (1 << 28)) throw Refuse("a CIGAR operation of 2^28 or more");
    if (!r.cigar.empty() && (r.cigar.back() & 0xF) == op && (int64_t)(r.cigar.back() >> 4) + len < (1 << 28)) r.cigar.back() += (uint32_t)len << 4;
    else r.cigar.push_back((uint32_t)len << 4 | op);
}

inline uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

struct SliceHeader { int32_t ref = -1, start = 0, span = 0, n_records = 0; int64_t counter = 0; };

inline SliceHeader parse_slice_header(const uint8_t* p, size_t n)
{
    Bytes in;
    in.p = p;
    in.n = n;
    in.name = "slice header";
    SliceHeader s;
    s.ref = in.itf8();
    s.start = in.itf8();
    s.span = in.itf8();
    s.n_records = in.itf8();
    s.counter = in.ltf8();
    if (s.n_records < 0) throw Refuse("slice header: a negative number of records");
    return s;
}

struct Block { const uint8_t* p; size_t n; int32_t content_id; bool core; };

// The slice's records into `records` (BAM records side by side, block_size first) and `rec_off` (n + 1 offsets).
inline void decode_slice(const uint8_t* comp, size_t comp_len, const uint8_t* slice_hdr, size_t slice_len, const std::vector<Block>& blocks,
                         const std::vector<std::string>& rg_ids, int32_t n_ref, std::vector<uint8_t>& records, std::vector<uint64_t>& rec_off)
{
    Header h;
    parse_header(comp, comp_len, h);
    const SliceHeader sh = parse_slice_header(slice_hdr, slice_len);
    Slice s;
    for (const Block& b : blocks) {
        if (b.core) {
            s.core.p = b.p;
            s.core.n = b.n;
        } else {
            Bytes x;
            x.p = b.p;
            x.n = b.n;
            x.name = "external block " + std::to_string(b.content_id);
            s.ext[b.content_id] = x;
        }
    }
    for (auto& kv : h.series) s.bind(kv.second);
    for (auto& kv : h.tags) s.bind(kv.second);
    auto ser = [&](const char* key) -> Codec& {
        Codec& c = h.series[key];
        if (c.series.empty()) c.series = key;
        return c;
    };
    Codec &BF = ser("BF"), &CF = ser("CF"), &RI = ser("RI"), &RL = ser("RL"), &AP = ser("AP"), &RG = ser("RG"), &RN = ser("RN"), &MF = ser("MF"),
          &NS = ser("NS"), &NP = ser("NP"), &TS = ser("TS"), &NF = ser("NF"), &TL = ser("TL"), &FN = ser("FN"), &FC = ser("FC"), &FP = ser("FP"),
          &DL = ser("DL"), &BA = ser("BA"), &QS = ser("QS"), &BS = ser("BS"), &IN = ser("IN"), &SC = ser("SC"), &HC = ser("HC"), &PD = ser("PD"),
          &RS = ser("RS"), &BB = ser("BB"), &QQ = ser("QQ"), &MQ = ser("MQ");

    const size_t n = (size_t)sh.n_records;
    if (n > (1u << 24)) throw Refuse("slice header: more than 2^24 records in one slice");
    std::vector<Rec> recs(n);
    int64_t last_pos = sh.start;
    std::vector<uint8_t> tmp;
    for (size_t i = 0; i < n; ++i) {
        Rec& r = recs[i];
        r.flag = s.value(BF, false);
        r.cf = s.value(CF, false);
        r.ref = sh.ref == -2 ? s.value(RI, false) : sh.ref;
        if (r.ref < -1 || r.ref >= n_ref) throw Refuse("a record on reference " + std::to_string(r.ref) + ", which the header does not have");
        r.rl = s.value(RL, false);
        if (r.rl < 0) throw Refuse("a record of negative read length");
        int64_t ap = s.value(AP, false);
        if (h.ap_delta) {
            ap += last_pos;
            last_pos = ap;
        }
        if (ap < 0 || ap > 0x7FFFFFFF) throw Refuse("a record position out of range");
        r.pos = (int32_t)ap - 1;
        r.rg = s.value(RG, false);
        if (r.rg < -1 || r.rg >= (int32_t)rg_ids.size()) throw Refuse("a record of read group " + std::to_string(r.rg) + ", which the header does not have");
        bool named = false;
        if (h.names) {
            tmp.clear();
            s.array(RN, &tmp);
            r.name.assign(tmp.begin(), tmp.end());
            named = true;
        }
        if (r.cf & 2) {                                      // detached
            const int32_t mf = s.value(MF, false);
            if (!h.names) {
                tmp.clear();
                s.array(RN, &tmp);
                r.name.assign(tmp.begin(), tmp.end());
                named = true;
            }
            r.next_ref = s.value(NS, false);
            if (r.next_ref < -1 || r.next_ref >= n_ref) throw Refuse("a mate on reference " + std::to_string(r.next_ref) + ", which the header does not have");
            r.next_pos = s.value(NP, false) - 1;
            r.tlen = s.value(TS, false);
            if (mf & 1) r.flag |= 0x20;
            if (mf & 2) r.flag |= 0x8;
        } else if (r.cf & 4) {                               // the mate is further down in this slice
            r.nf = s.value(NF, false);
            if (r.nf < 0 || (size_t)r.nf >= n - i - 1) throw Refuse("a record whose mate (NF) lies outside its slice");
            r.next = (int64_t)i + r.nf + 1;
        }
        if (!named) r.name.clear();                          // (named by its chain's first, below)
        else if (r.name.empty()) r.name = "*";
        // tags
        const int32_t tl = s.value(TL, false);
        if (tl < 0 || (size_t)tl >= h.tag_lists.size()) {
            if (!(tl == 0 && h.tag_lists.empty())) throw Refuse("a record whose tag list (TL) is not in the TD dictionary");
        } else {
            for (const uint32_t id : h.tag_lists[(size_t)tl]) {
                auto it = h.tags.find(id);
                if (it == h.tags.end()) throw Refuse("a tag of the TD dictionary has no encoding");
                r.aux.push_back((uint8_t)(id >> 16));
                r.aux.push_back((uint8_t)(id >> 8));
                r.aux.push_back((uint8_t)id);
                s.array(it->second, &r.aux);
            }
        }
        int64_t ref_len = 0;
        if (!(r.flag & 0x4)) {
            const int32_t fn = s.value(FN, false);
            if (fn < 0) throw Refuse("a record with a negative number of features");
            int64_t read_pos = 1, fp = 0;
            for (int32_t f = 0; f < fn; ++f) {
                const int32_t code = s.value(FC, true);
                fp += s.value(FP, false);
                if (fp > read_pos) {
                    add_op(r, 0, fp - read_pos);
                    ref_len += fp - read_pos;
                    read_pos = fp;
                }
                int64_t len;
                switch (code) {
                case 'B':
                    (void)s.value(BA, true);
                    (void)s.value(QS, true);
                    add_op(r, 0, 1); ++ref_len; ++read_pos;
                    break;
                case 'X':
                    (void)s.value(BS, true);
                    add_op(r, 0, 1); ++ref_len; ++read_pos;
                    break;
                case 'b':
                    len = (int64_t)s.array(BB, nullptr);
                    add_op(r, 0, len); ref_len += len; read_pos += len;
                    break;
                case 'I':
                    len = (int64_t)s.array(IN, nullptr);
                    add_op(r, 1, len); read_pos += len;
                    break;
                case 'i':
                    (void)s.value(BA, true);
                    add_op(r, 1, 1); ++read_pos;
                    break;
                case 'S':
                    len = (int64_t)s.array(SC, nullptr);
                    add_op(r, 4, len); read_pos += len;
                    break;
                case 'D': len = s.value(DL, false); add_op(r, 2, len); ref_len += len > 0 ? len : 0; break;
                case 'N': len = s.value(RS, false); add_op(r, 3, len); ref_len += len > 0 ? len : 0; break;
                case 'H': add_op(r, 5, s.value(HC, false)); break;
                case 'P': add_op(r, 6, s.value(PD, false)); break;
                case 'q': (void)s.array(QQ, nullptr); break;
                case 'Q': (void)s.value(QS, true); break;
                default: throw Refuse("a read feature of unknown code " + std::to_string(code));
                }
            }
            if (read_pos <= r.rl) {
                add_op(r, 0, (int64_t)r.rl - read_pos + 1);
                ref_len += (int64_t)r.rl - read_pos + 1;
            }
            r.mapq = s.value(MQ, false);
            if (r.cf & 1)
                for (int32_t k = 0; k < r.rl; ++k) (void)s.value(QS, true);
        } else {
            if (!(r.cf & 8))
                for (int32_t k = 0; k < r.rl; ++k) (void)s.value(BA, true);
            if (r.cf & 1)
                for (int32_t k = 0; k < r.rl; ++k) (void)s.value(QS, true);
        }
        r.end = (int64_t)r.pos + (ref_len > 0 ? ref_len : 1);
        if (r.cigar.size() > 0xFFFF) throw Refuse("a record of more than 65535 CIGAR operations");
        if (r.mapq < 0 || r.mapq > 255) throw Refuse("a mapping quality out of range");
    }
    // chains of attached records
    std::vector<uint8_t> targeted(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (recs[i].next >= 0) {
            if (targeted[(size_t)recs[i].next]) throw Refuse("two records name the same mate (NF)");
            targeted[(size_t)recs[i].next] = 1;
        }
    for (size_t i = 0; i < n; ++i) {
        if (targeted[i] || recs[i].next < 0) {
            if (!targeted[i] && recs[i].name.empty()) recs[i].name = std::to_string(sh.counter + (int64_t)i);
            continue;
        }
        // i is the first of a chain
        int64_t lo = 0, hi = 0, first = (int64_t)i;
        bool spans = true;
        size_t leftmost = i;
        for (int64_t k = first; k >= 0; k = recs[(size_t)k].next) {
            Rec& r = recs[(size_t)k];
            r.head = first;
            if ((r.flag & 0x4) || r.ref < 0 || r.ref != recs[i].ref) spans = false;
            if (k == first || r.pos < lo) {
                if (k != first) leftmost = (size_t)k;
                lo = r.pos;
            }
            if (k == first || r.end > hi) hi = r.end;
        }
        const std::string name = recs[i].name.empty() ? std::to_string(sh.counter + (int64_t)i) : recs[i].name;
        for (int64_t k = first; k >= 0; k = recs[(size_t)k].next) {
            Rec& r = recs[(size_t)k];
            const Rec& mate = recs[(size_t)(r.next >= 0 ? r.next : first)];
            if (r.name.empty()) r.name = name;
            r.next_ref = mate.ref;
            r.next_pos = mate.pos;
            r.flag &= ~(0x20 | 0x8);
            if (mate.flag & 0x10) r.flag |= 0x20;
            if (mate.flag & 0x4) r.flag |= 0x8;
            const int64_t span = hi - lo;
            if (span > 0x7FFFFFFF) throw Refuse("a template length out of range");
            r.tlen = !spans ? 0 : (size_t)k == leftmost ? (int32_t)span : -(int32_t)span;
        }
    }
    // BAM records
    records.clear();
    rec_off.assign(1, 0);
    auto put32 = [&](uint32_t v) {
        for (int k = 0; k < 4; ++k) records.push_back((uint8_t)(v >> (8 * k)));
    };
    for (size_t i = 0; i < n; ++i) {
        const Rec& r = recs[i];
        if (r.name.size() > 254) throw Refuse("a read name of more than 254 characters");
        std::vector<uint8_t> rg;
        if (r.rg >= 0) {
            const std::string& id = rg_ids[(size_t)r.rg];
            rg.assign({'R', 'G', 'Z'});
            rg.insert(rg.end(), id.begin(), id.end());
            rg.push_back(0);
        }
        const size_t l_name = r.name.size() + 1, l_seq = (r.cf & 8) ? 0 : (size_t)r.rl;    // (CF bit 8: the record has no sequence, `*`)
        const size_t size = 32 + l_name + 4 * r.cigar.size() + (l_seq + 1) / 2 + l_seq + rg.size() + r.aux.size();
        if (size > 0x7FFFFFFFull) throw Refuse("a record of 2 GiB or more");
        put32((uint32_t)size);
        put32((uint32_t)r.ref);
        put32((uint32_t)r.pos);
        const uint32_t bin = reg2bin(r.pos < 0 ? -1 : r.pos, r.pos < 0 ? 0 : r.end);
        put32((uint32_t)l_name | (uint32_t)r.mapq << 8 | bin << 16);
        put32((uint32_t)r.cigar.size() | (uint32_t)(r.flag & 0xFFFF) << 16);
        put32((uint32_t)l_seq);
        put32((uint32_t)r.next_ref);
        put32((uint32_t)r.next_pos);
        put32((uint32_t)r.tlen);
        records.insert(records.end(), r.name.begin(), r.name.end());
        records.push_back(0);
        for (const uint32_t c : r.cigar) put32(c);
        records.insert(records.end(), (l_seq + 1) / 2, (uint8_t)0xFF);
        if (l_seq & 1) records.back() = 0xF0;
        records.insert(records.end(), l_seq, (uint8_t)0xFF);
        records.insert(records.end(), rg.begin(), rg.end());
        records.insert(records.end(), r.aux.begin(), r.aux.end());
        rec_off.push_back(records.size());
    }
}

}  // namespace cram
}  // namespace svt

#endif  // SVT_CRAM_H

"""An independent BCF2.2 reader in plain Python, written from the published format (VCFv4.3 specification, section 6): the header,
the implicit dictionaries, and every record back to VCF fields.  Nothing here imports svtyper_amd: this is the yardstick the
package's encoder is held against.

A decoded record is a dict of the VCF columns with values in a canonical form that a VCF data line is brought into by
`line_fields` as well, so the two compare with ==:
    chrom, pos (1-based), id, ref, alt (list), qual (None or float32 bits), filter (None for '.', else a list of names),
    info: [(key, value)] in line order -- True for a Flag or a key without value, a list of ints / None for Integer, a list of
    float32 bit patterns / None for Float, a str for String; format: [keys]; samples: [[value per key]] with the same value forms,
    GT as a list of (allele or None, phased).
Floats compare bitwise: a text token t is numpy.float32(float(t)), the double nearest the decimal text rounded to float32."""
import re
import struct
import zlib

import numpy as np

EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
INT_MISSING = {1: -128, 2: -32768, 3: -2147483648}
INT_EOV = {1: -127, 2: -32767, 3: -2147483647}
INT_FMT = {1: "b", 2: "h", 3: "i"}
FLOAT_MISSING, FLOAT_EOV = 0x7F800001, 0x7F800002


# ------------------------------------------------------------------------------------------ BGZF
def members(data):
    """[(file offset, where its payload begins in the stream, payload)] of the BGZF file `data`, the EOF member required and left out"""
    assert data.endswith(EOF), "no BGZF EOF member"
    out, at, start = [], 0, 0
    while at < len(data) - len(EOF):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\0", "not a BGZF member at %d" % at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        payload = zlib.decompress(data[at + 18:at + size - 8], -15)
        crc, isize = struct.unpack_from("<II", data, at + size - 8)
        assert zlib.crc32(payload) & 0xFFFFFFFF == crc and len(payload) == isize
        out.append((at, start, payload))
        start += len(payload)
        at += size
    return out


def stream_of(data):
    return b"".join(m[2] for m in members(data))


def position(mem, voff, file_len):
    """where the virtual offset `voff` points in the stream"""
    coff, uoff = voff >> 16, voff & 0xFFFF
    for at, start, payload in mem:
        if at == coff:
            assert uoff < len(payload) or (uoff == 0 and not payload)
            return start + uoff
    assert coff == file_len - len(EOF) and uoff == 0, "a virtual offset into no member"
    return sum(len(m[2]) for m in mem)


# ------------------------------------------------------------------------------------------ the header
def header_field(line, field):
    m = re.search(r'[<,]%s=("[^"]*"|[^,>]*)' % field, line)
    return m.group(1) if m else None


def read_header(stream):
    """-> (header text, {"strings": [names], "types": {(category, name): Type}, "contigs": [names], "lengths": [..], "samples": [names]}, where the records begin)"""
    assert stream[:5] == b"BCF\2\2", "no BCF2.2 magic"
    l_text = struct.unpack_from("<I", stream, 5)[0]
    raw = stream[9:9 + l_text]
    assert raw.endswith(b"\0") and b"\0" not in raw[:-1], "the header text is NUL-terminated once"
    text = raw[:-1].decode("utf-8")
    strings, types, contigs, lengths, samples = ["PASS"], {("FILTER", "PASS"): "Filter"}, [], [], []
    for line in text.split("\n"):
        for cat in ("FILTER", "INFO", "FORMAT"):
            if line.startswith("##%s=<" % cat):
                assert "IDX=" not in line
                name = header_field(line, "ID")
                if name not in strings:
                    strings.append(name)
                types.setdefault((cat, name), header_field(line, "Type") or "Filter")
        if line.startswith("##contig=<"):
            name = header_field(line, "ID")
            if name not in contigs:
                contigs.append(name)
                lengths.append(int(header_field(line, "length") or 0))
        if line.startswith("#CHROM"):
            samples = line.split("\t")[9:]
    return text, dict(strings=strings, types=types, contigs=contigs, lengths=lengths, samples=samples), 9 + l_text


# ------------------------------------------------------------------------------------------ typed values
def read_descriptor(buf, at):
    """-> (type, count, at)"""
    b = buf[at]
    at += 1
    kind, count = b & 15, b >> 4
    if count == 15:
        t2, c2, at = read_descriptor(buf, at)
        assert c2 == 1 and t2 in INT_FMT
        count = struct.unpack_from("<" + INT_FMT[t2], buf, at)[0]
        at += struct.calcsize(INT_FMT[t2])
        assert count >= 15, "a long count for a short vector"
    return kind, count, at


def read_values(buf, at, kind, count):
    """-> (raw values, at): ints for 1..3, uint32 bit patterns for 5, bytes for 7"""
    if kind in INT_FMT:
        size = struct.calcsize(INT_FMT[kind])
        return list(struct.unpack_from("<%d%s" % (count, INT_FMT[kind]), buf, at)), at + size * count
    if kind == 5:
        return list(struct.unpack_from("<%dI" % count, buf, at)), at + 4 * count
    if kind == 7:
        return bytes(buf[at:at + count]), at + count
    assert kind == 0 and count == 0, "type %d" % kind
    return None, at


def read_typed(buf, at):
    kind, count, at = read_descriptor(buf, at)
    values, at = read_values(buf, at, kind, count)
    return kind, values, at


def smallest_int_type(values):
    present = [v for v in values]
    if all(-120 <= v <= 127 for v in present):
        return 1
    if all(-32760 <= v <= 32767 for v in present):
        return 2
    return 3


def int_vector(kind, raw):
    """a vector of width `kind` -> ints / None, its end-of-vector tail cut; the width must be the smallest that holds the values"""
    out, ended = [], False
    for v in raw:
        if v == INT_EOV[kind]:
            ended = True
            continue
        assert not ended, "a value behind end-of-vector"
        out.append(None if v == INT_MISSING[kind] else v)
    return out


def float_vector(raw):
    out, ended = [], False
    for v in raw:
        if v == FLOAT_EOV:
            ended = True
            continue
        assert not ended, "a value behind end-of-vector"
        out.append(None if v == FLOAT_MISSING else v)
    return out


def gt_vector(kind, raw):
    return [(None if v >> 1 == 0 else (v >> 1) - 1, bool(v & 1)) for v in int_vector(kind, raw)]


# ------------------------------------------------------------------------------------------ records
def read_record(stream, at, d):
    """-> (record dict, where the next record begins)"""
    l_shared, l_indiv = struct.unpack_from("<II", stream, at)
    shared = memoryview(stream)[at + 8:at + 8 + l_shared]
    indiv = memoryview(stream)[at + 8 + l_shared:at + 8 + l_shared + l_indiv]
    assert len(shared) == l_shared and len(indiv) == l_indiv, "a record runs out of the stream"
    chrom, pos0, rlen, qual, n_allele_info, n_fmt_sample = struct.unpack_from("<iiiIII", shared, 0)
    n_allele, n_info, n_fmt, n_sample = n_allele_info >> 16, n_allele_info & 0xFFFF, n_fmt_sample >> 24, n_fmt_sample & 0xFFFFFF
    assert 0 <= chrom < len(d["contigs"]) and n_sample == len(d["samples"])
    p = 24
    kind, ident, p = read_typed(shared, p)
    assert kind == 7
    alleles = []
    for _ in range(n_allele):
        kind, a, p = read_typed(shared, p)
        assert kind == 7
        alleles.append(a.decode())
    kind, filt, p = read_typed(shared, p)
    assert kind in (0, 1, 2, 3)
    if filt is not None:
        assert kind == smallest_int_type(filt), "FILTER is not in its smallest width"
    info = []
    for _ in range(n_info):
        kk, key, p = read_typed(shared, p)
        assert kk in INT_FMT and len(key) == 1 and kk == smallest_int_type(key)
        name = d["strings"][key[0]]
        declared = d["types"][("INFO", name)]
        kind, raw, p = read_typed(shared, p)
        if raw is None:
            value = True
        elif declared == "Integer":
            assert kind in INT_FMT
            value = int_vector(kind, raw)
            assert len(value) == len(raw), "an INFO vector is not padded"
            assert kind == smallest_int_type([v for v in value if v is not None]), "%s is not in its smallest width" % name
        elif declared == "Float":
            assert kind == 5
            value = float_vector(raw)
        else:
            assert kind == 7 and declared in ("String", "Character")
            value = raw.decode()
        info.append((name, value))
    assert p == l_shared, "l_shared is not the shared part's length"
    fmt, columns, p = [], [], 0
    for _ in range(n_fmt):
        kk, key, p = read_typed(indiv, p)
        assert kk in INT_FMT and len(key) == 1 and kk == smallest_int_type(key)
        name = d["strings"][key[0]]
        declared = d["types"][("FORMAT", name)]
        kind, count, p = read_descriptor(indiv, p)
        per_sample = []
        widest = 0
        present = []
        for _s in range(n_sample):
            raw, p = read_values(indiv, p, kind, count)
            if name == "GT":
                assert kind in INT_FMT
                value = gt_vector(kind, raw)
                present += [v for v in raw if v != INT_EOV[kind]]
                widest = max(widest, len(value))
            elif declared == "Integer":
                assert kind in INT_FMT
                value = int_vector(kind, raw)
                present += [v for v in value if v is not None]
                widest = max(widest, len(value))
            elif declared == "Float":
                assert kind == 5
                value = float_vector(raw)
                widest = max(widest, len(value))
            else:
                assert kind == 7
                value = raw.rstrip(b"\0")
                assert b"\0" not in value
                widest = max(widest, len(value))
                value = value.decode()
            per_sample.append(value)
        assert widest == count, "%s: the count is not the longest vector" % name
        if kind in INT_FMT:
            assert kind == smallest_int_type(present), "%s is not in its smallest width" % name
        fmt.append(name)
        columns.append(per_sample)
    assert p == l_indiv, "l_indiv is not the individual part's length"
    rec = dict(chrom=d["contigs"][chrom], pos=pos0 + 1, id=ident.decode() if ident else ".", ref=alleles[0], alt=alleles[1:],
               qual=None if qual == FLOAT_MISSING else qual, filter=None if filt is None else [d["strings"][k] for k in filt], info=info,
               format=fmt, samples=[[col[s] for col in columns] for s in range(n_sample)], rlen=rlen)
    return rec, at + 8 + l_shared + l_indiv


def read_bcf(stream):
    """-> (header text, dictionaries, [record], [where each record begins])"""
    text, d, at = read_header(stream)
    records, offsets = [], []
    while at < len(stream):
        offsets.append(at)
        rec, at = read_record(stream, at, d)
        records.append(rec)
    assert at == len(stream)
    return text, d, records, offsets


# ------------------------------------------------------------------------------------------ the same fields from VCF text
def float_bits(token):
    with np.errstate(over="ignore"):                # (a double beyond float32's range is an infinity, as the C cast makes it)
        return int(np.float32(float(token)).view(np.uint32))


def _ints(token):
    return [None if t == "." else int(t) for t in token.split(",")]


def _floats(token):
    return [None if t == "." else float_bits(t) for t in token.split(",")]


def _gt(token):
    out, phased = [], False
    for part in re.split(r"([/|])", token):
        if part in ("/", "|"):
            phased = part == "|"
        else:
            out.append((None if part == "." else int(part), phased))
    return out


def line_fields(line, d):
    """the data line `line` (str, no newline) in read_record's form; `d`: the dictionaries of read_header"""
    cols = line.split("\t")
    info = []
    end = None
    if cols[7] != ".":
        for item in cols[7].split(";"):
            if not item:
                continue
            key, eq, value = item.partition("=")
            declared = d["types"][("INFO", key)]
            if not eq or declared == "Flag":
                info.append((key, True))
            elif declared == "Integer":
                info.append((key, _ints(value)))
                if key == "END" and end is None:
                    end = _ints(value)[0]
            elif declared == "Float":
                info.append((key, _floats(value)))
            else:
                info.append((key, value))
    fmt = cols[8].split(":") if len(cols) > 8 else []
    samples = []
    for column in cols[9:]:
        parts = column.split(":")
        row = []
        for k, key in enumerate(fmt):
            declared = d["types"][("FORMAT", key)]
            token = parts[k] if k < len(parts) else None
            if key == "GT":
                row.append(_gt(token if token is not None else "."))
            elif declared == "Integer":
                row.append(_ints(token) if token is not None else [None])
            elif declared == "Float":
                row.append(_floats(token) if token is not None else [None])
            else:
                row.append(token if token is not None else ".")
        samples.append(row)
    if len(cols) <= 8:
        samples = [[] for _ in d["samples"]]
    pos = int(cols[1])
    rlen = end - (pos - 1) if end is not None and end > pos - 1 else len(cols[3])
    return dict(chrom=cols[0], pos=pos, id=cols[2], ref=cols[3], alt=[] if cols[4] == "." else cols[4].split(","),
                qual=None if cols[5] == "." else float_bits(cols[5]), filter=None if cols[6] == "." else cols[6].split(";"), info=info,
                format=fmt, samples=samples, rlen=rlen)

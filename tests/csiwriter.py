"""Test helper: write the CSI index (CSIv1, what `samtools index -c -m MIN_SHIFT` writes) of a coordinate-sorted BAM, for any
binning scheme (min_shift, depth).  Independent of the readers under test: the BAM is inflated here with zlib and its record
chain walked with struct.

  bins      a record goes into the smallest bin of the scheme that holds [pos, end); a bin's chunks follow
            tests/bamwriter.py::write_bam's rule -- a chunk grows while the next record of the bin starts where the last ended
  loffset   of a bin: the virtual offset of the first record of that reference, in file order, that ends behind the bin's start
            (no record that overlaps a position of the bin lies in front of it)
  pseudo-bin  (8^(depth+1) - 1) / 7 + 1 of every reference that has records: [offset of its first record, offset behind its
            last], [mapped, unmapped]; behind the references n_no_coor, the reads without a reference

A virtual offset is bamwriter's: block offset << 16 | offset in the block, and the start of the next block for a position at a
block's end (the end of the data: see voff).  The index is BGZF-compressed in members of at most `member_bytes` (64 KiB at most)."""
import bisect
import struct
import zlib

import bamwriter as bw


def inflate_bam(path):
    """(the inflated stream, [(stream position of a block's first byte, its file offset)] of the non-empty blocks, file offset of
    the first block behind the data)"""
    raw = open(path, "rb").read()
    parts, blocks, at, coff = [], [], 0, 0
    end_coff = None
    while coff + 18 <= len(raw):
        assert raw[coff] == 31 and raw[coff + 1] == 139, "not a BGZF block at %d" % coff
        xlen = struct.unpack_from("<H", raw, coff + 10)[0]
        bsize, i = None, 0
        while i + 4 <= xlen:
            si1, si2, slen = raw[coff + 12 + i], raw[coff + 13 + i], struct.unpack_from("<H", raw, coff + 14 + i)[0]
            if si1 == 66 and si2 == 67:
                bsize = struct.unpack_from("<H", raw, coff + 16 + i)[0]
            i += 4 + slen
        data = zlib.decompress(raw[coff + 12 + xlen:coff + bsize + 1 - 8], -15)
        if data:
            blocks.append((at, coff))
            parts.append(data)
            at += len(data)
            end_coff = None
        elif end_coff is None:
            end_coff = coff
        coff += bsize + 1
    return b"".join(parts), blocks, (coff if end_coff is None else end_coff)


def reg2bin(beg, end, min_shift, depth):
    """the smallest bin that holds [beg, end) (CSIv1 spec)"""
    end -= 1
    s, t = min_shift, ((1 << (3 * depth)) - 1) // 7
    for l in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (l - 1))
    return 0


def bin_start(b, min_shift, depth):
    """the first position of bin `b`"""
    l = 0
    while ((1 << (3 * (l + 1))) - 1) // 7 <= b:
        l += 1
    return (b - ((1 << (3 * l)) - 1) // 7) << (min_shift + 3 * (depth - l))


def records_of(stream):
    """(n_ref, [(stream start, stream end, tid, pos, end, flag)]) of the BAM's record chain"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    out = []
    while at + 4 <= len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        tid, pos, l_name, _mapq, _bin, n_cigar, flag = struct.unpack_from("<iiBBHHH", stream, at + 4)
        cigar = struct.unpack_from("<%dI" % n_cigar, stream, at + 36 + l_name)
        ref = sum(c >> 4 for c in cigar if (c & 0xF) in (0, 2, 3, 7, 8))
        out.append((at, at + 4 + size, tid, pos, pos + max(1, ref), flag))
        at += 4 + size
    assert at == len(stream), "the record chain does not end with the data"
    return n_ref, out


def csi_bytes(bam_path, min_shift, depth, aux=b"", counts=True):
    stream, blocks, end_coff = inflate_bam(bam_path)
    starts = [a for a, _ in blocks]

    def voff(p):
        if p >= len(stream):
            # the end of the data, as bamwriter.write_bam puts it: behind the last byte of a last block that is shorter than the
            # blocks in front of it, else the start of the block behind the data
            last = len(stream) - blocks[-1][0]
            short = len(blocks) == 1 or last < blocks[1][0] - blocks[0][0]
            return (blocks[-1][1] << 16) | last if short else end_coff << 16
        k = bisect.bisect_right(starts, p) - 1
        return (blocks[k][1] << 16) | (p - blocks[k][0])

    n_ref, recs = records_of(stream)
    assert all(end <= 1 << (min_shift + 3 * depth) for _s, _e, tid, _p, end, _f in recs if tid >= 0), "the scheme does not cover the records"
    bins = [dict() for _ in range(n_ref)]
    order = [[] for _ in range(n_ref)]              # per reference, in file order: (running maximum of the ends, offset)
    stats = [[None, None, 0, 0] for _ in range(n_ref)]
    n_no_coor = 0
    for s, e, tid, pos, end, flag in recs:
        if tid < 0:
            n_no_coor += 1
            continue
        v0, v1 = voff(s), voff(e)
        chunks = bins[tid].setdefault(reg2bin(pos, end, min_shift, depth), [])
        if chunks and chunks[-1][1] == v0:
            chunks[-1][1] = v1
        else:
            chunks.append([v0, v1])
        order[tid].append((max(end, order[tid][-1][0]) if order[tid] else end, v0))
        st = stats[tid]
        st[0] = v0 if st[0] is None else st[0]
        st[1] = v1
        st[3 if flag & 0x4 else 2] += 1
    pseudo = ((1 << (3 * (depth + 1))) - 1) // 7 + 1
    out = b"CSI\1" + struct.pack("<iii", min_shift, depth, len(aux)) + aux + struct.pack("<i", n_ref)
    for tid in range(n_ref):
        ends = [m for m, _ in order[tid]]
        n_bin = len(bins[tid]) + (1 if counts and order[tid] else 0)
        out += struct.pack("<i", n_bin)
        for b, chunks in sorted(bins[tid].items()):
            k = bisect.bisect_right(ends, bin_start(b, min_shift, depth))      # the first record that ends behind the bin's start
            out += struct.pack("<IQi", b, order[tid][k][1], len(chunks)) + b"".join(struct.pack("<QQ", c0, c1) for c0, c1 in chunks)
        if counts and order[tid]:
            st = stats[tid]
            out += struct.pack("<IQi", pseudo, 0, 2) + struct.pack("<QQQQ", st[0], st[1], st[2], st[3])
    if counts:
        out += struct.pack("<Q", n_no_coor)
    return out


def bgzf(data, member_bytes=0xff00):
    assert 0 < member_bytes <= 65536
    return b"".join(bw.bgzf_block(data[i:i + member_bytes]) for i in range(0, len(data), member_bytes)) + bw.BGZF_EOF


def write_csi(bam_path, csi_path, min_shift, depth, aux=b"", member_bytes=0xff00, counts=True):
    """the CSI of `bam_path` in the scheme (min_shift, depth) at `csi_path`; `aux`: the l_aux bytes behind the header"""
    with open(csi_path, "wb") as f:
        f.write(bgzf(csi_bytes(bam_path, min_shift, depth, aux, counts), member_bytes))
    return csi_path

"""Inputs shared by tests/test_csi_index_host.py (CPU) and tests/test_csi_index_device.py (GPU): the BAMs of tests/walkcases.py,
each copied to a directory of its own WITHOUT its .bai and indexed as CSI by tests/csiwriter.py in several binning schemes, and
the long-contig groups of tests/golden/long_contig_sites.json.gz (made by the reference: make_golden_long_contig.py) written as
BAMs whose positions only a CSI of depth 6 addresses."""
import copy
import os
import shutil
import struct
from unittest import mock

import bamwriter as bw
import csiwriter
import goldenio as gio
import walkcases as W
from svtyper_amd import bam, native_reads as nr

# (min_shift, depth): every scheme covers the longest contig of the files it is used on.  (14, 5) is the BAI's own; (14, 6)
# what samtools takes beyond 512 Mbp; (16, 5) has leaves four times wider, (13, 6) leaves half as wide under one more level;
# (10, 3) ends at 2^19, behind the 400-kbp contigs of the synthetic and fake BAMs.
FIXTURE_SHAPES = ((14, 5), (14, 6), (16, 5), (13, 6))
SMALL_SHAPES = FIXTURE_SHAPES + ((10, 3),)
LONG_SHAPE = (14, 6)
LONG_GOLDEN = "long_contig_sites.json.gz"


def csi_only_copy(src_bam, directory, shape, name=None, **kw):
    """`src_bam` copied into `directory` (created) with a .csi of `shape` and no .bai; the copy's path"""
    os.makedirs(str(directory), exist_ok=True)
    dst = os.path.join(str(directory), name or os.path.basename(src_bam))
    shutil.copy(src_bam, dst)
    assert not os.path.exists(dst + ".bai") and not os.path.exists(os.path.splitext(dst)[0] + ".bai")
    csiwriter.write_csi(dst, dst + ".csi", shape[0], shape[1], **kw)
    return dst


def on_copy(sample, path):
    """(the sample with its Python reader on `path`, the native reader on `path`)"""
    s = copy.copy(sample)
    s.bam = bam.AlignmentFile(path)
    return s, nr.NativeBam(path)


def walk_inputs(tmp_path):
    """(label, sites, sample, nbam, shapes) of the BAMs of walkcases, BAI-indexed as they are: the fixture, synthetic seeds 11 and
    12, fake group 0 and the three-BAM golden inputs"""
    sites, sample, nbam = W.fixture_input()
    yield "fixture", sites, sample, nbam, FIXTURE_SHAPES
    for seed in (11, 12):
        sites, sample, nbam = W.synthetic_input(tmp_path, seed)
        yield "syn%d" % seed, sites, sample, nbam, SMALL_SHAPES
    sites, sample, nbam = next(iter(W.fake_inputs(tmp_path)))
    yield "fake0", sites, sample, nbam, SMALL_SHAPES
    for k, (sites, sample, nbam) in enumerate(W.three_bam_inputs(tmp_path)):
        yield "three%d" % k, sites, sample, nbam, SMALL_SHAPES


def write_bam_without_bai(path, header_text, references, records, block_bytes):
    """The BAM of bamwriter.write_bam -- its record encoder, its blocks cut at `block_bytes` whatever the records, its EOF block --
    and no .bai.  write_bam itself is not used at these positions: its .bai gets one linear entry per 16 kbp up to the last read,
    131 072 of them appended one by one (tens of seconds for nothing), and beyond 997 Mbp the BAI bin number it puts into a
    record no longer fits the record's 16-bit field.  That field says nothing beyond 2^29 and no reader here looks at it: it is
    cut to 16 bits, as htslib cuts it."""
    text = header_text.encode()
    parts = [b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(references))]
    for name, length in references:
        nm = name.encode() + b"\0"
        parts.append(struct.pack("<i", len(nm)) + nm + struct.pack("<i", length))
    plain = bw.reg2bin
    with mock.patch.object(bw, "reg2bin", lambda beg, end: plain(beg, end) & 0xFFFF):
        parts += [bw.encode_record(r)[0] for r in records]
    stream = b"".join(parts)
    with open(path, "wb") as f:
        f.write(b"".join(bw.bgzf_block(stream[i:i + block_bytes]) for i in range(0, len(stream), block_bytes)) + bw.BGZF_EOF)


def long_contig_groups(tmp_path):
    """[(group of the golden, sites, sample, nbam)]: every group written as bamwriter.write_bam writes a BAM, without a .bai (a
    BAI says nothing at these positions), and indexed as CSI (14, 6)"""
    g = gio.load(LONG_GOLDEN)
    n = g["ref_length"]
    refs = [("1", n), ("2", n)]
    tid_of = {"1": 0, "2": 1}
    out = []
    for k, group in enumerate(g["groups"]):
        libs = group["libraries"]
        header = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:%d\n@SQ\tSN:2\tLN:%d\n" % (n, n) + "".join(
            "@RG\tID:%s\tSM:long\tLB:%s\n" % (rg, L["name"]) for L in libs for rg in L["readgroups"])
        recs = []
        for site in group["sites"]:
            for (name, flag, ref, start, cigar, mapq, sa, rg, _qlen, tlen) in site["reads"]:
                tags = [("RG", "Z", rg)] + ([("SA", "Z", sa)] if sa else [])
                recs.append(dict(name=name, flag=flag, tid=tid_of[ref], pos=start, mapq=mapq, cigar=cigar, mtid=tid_of[ref],
                                 mpos=start, tlen=tlen, tags=tags))
        recs.sort(key=lambda r: (r["tid"], r["pos"]))
        path = os.path.join(str(tmp_path), "long%d.bam" % k)
        write_bam_without_bai(path, header, refs, recs, block_bytes=2300 + 400 * k)
        csiwriter.write_csi(path, path + ".csi", *LONG_SHAPE)
        info = {"long": {"mapped": len(recs), "unmapped": 0, "bam": path, "sample_name": "long", "libraryArray": [
            {"library_name": L["name"], "readgroups": L["readgroups"], "read_length": L["read_length"], "histogram": L["hist"],
             "mean": gio.fh(L["mean"]), "sd": gio.fh(L["sd"]), "prevalence": 1.0 / len(libs)} for L in libs]}}
        sample, nbam = W.open_sample(path, info)
        out.append((group, [{"breakpoint": s["breakpoint"]} for s in group["sites"]], sample, nbam))
    return out

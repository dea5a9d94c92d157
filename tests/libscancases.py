"""Test helper: the BAMs and the comparison of the library-scan tests (tests/test_library_walk_host.py on the CPU,
tests/test_library_scan_device.py on the GPU).  The reference of every case is svt_bam_scan_library, library by library: the
walk must give the same keys in the same order with the same counts, the same read length, in_lib and total -- or, outside
its envelope, a nonzero host_reason and the host scan's result or error."""
import os
import random
import shutil

import bamwriter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "data", "NA12878.target_loci.sorted.bam")
SMALL_ROUND = 256 << 10
WALK = "walk"                                 # compare(expect_reason=WALK): the walk itself answered
FIXTURE_NUM_SAMP = (1, 5000, 21277, 21278, 1000000, 0)

HEADER = ("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:3000000\n@SQ\tSN:c2\tLN:3000000\n@SQ\tSN:c3\tLN:3000000\n"
          "@RG\tID:r0\tSM:s\tLB:A\n@RG\tID:r1\tSM:s\tLB:B\n@RG\tID:r2\tSM:s\tLB:A\n@RG\tID:r3\tSM:s\n@RG\tID:r4\tSM:s\tLB:B\n"
          "@RG\tID:r5\tSM:s\tLB:Z\n")
REFS = [("c1", 3000000), ("c2", 3000000), ("c3", 3000000)]
# three libraries over five read groups, one of them without LB (library ""); r5 is in the file and in no library of the call
GROUPS = [["r0", "r2"], ["r1", "r4"], ["r3"]]
QUALIFYING = 0x1 | 0x2 | 0x20 | 0x40          # paired, mate reverse, first: a read of the histogram when tlen > 0


def capacities():
    from svtyper_amd import native_reads
    return native_reads.library_scan_capacities()


def synthetic_records(seed, n=3000, unplaced=5):
    """c1 and c3 hold the reads, c2 (in the middle) is empty; library B (r1, r4) is absent from the first half; template
    lengths repeat from window to window (one key first seen in many segments) and include K - 1, K, K + 1, 300 000,
    2^31 - 1, zero and negative ones; the file ends with unplaced reads, the last of them without RG."""
    rng = random.Random(seed)
    K = capacities()["dense_keys"]
    special = [K - 1, K, K + 1, 300000, 2 ** 31 - 1, 0, -250, K + 1, 300000, K - 1, 2 ** 31 - 1, K]
    recs, pos, tid = [], 100, 0
    for i in range(n):
        if i == n // 2:
            tid, pos = 2, 500
        pos += rng.randint(20, 400)
        rgs = ["r0", "r2", "r3", "r5"] if i < n // 2 else ["r0", "r1", "r2", "r3", "r4", "r5"]
        flag = QUALIFYING if rng.random() < 0.6 else rng.choice([0x1 | 0x10, 0x1 | 0x20 | 0x100, 0x1 | 0x20 | 0x800, 0x1 | 0x20 | 0x8,
                                                                 0x1 | 0x20 | 0x4, 0x1 | 0x20 | 0x10, 0x1])
        tlen = rng.randint(300, 340) if rng.random() < 0.9 else rng.choice([-rng.randint(1, 500), 0, rng.randint(341, 5000)])
        rg = rng.choice(rgs)
        if i % 211 == 7:                      # (15 of them in 3 000 records, 10 at or beyond K, all of library A)
            flag, tlen, rg = QUALIFYING, special[(i // 211) % len(special)], "r0"
        cigar = rng.choice(["100M", "5S95M", "40M2I58M", "30M5D70M", "101M", "20=3X77M10S", "60M40H", "*"])
        recs.append({"name": "q%05d" % i, "flag": flag, "tid": tid, "pos": pos, "mapq": 30, "cigar": cigar, "mtid": tid,
                     "mpos": pos + 200, "tlen": tlen,
                     "tags": [("NM", "C", 1), ("RG", "Z", rg), ("XS", "i", 5)]})
    for k in range(unplaced):
        tags = [("RG", "Z", "r0")] if k + 1 < unplaced else []
        recs.append({"name": "u%d" % k, "flag": 0x4, "tid": -1, "pos": -1, "mapq": 0, "cigar": "*", "mtid": -1, "mpos": -1, "tlen": 0, "tags": tags})
    return recs


def write_synthetic(path, seed, **kw):
    bamwriter.write_bam(path, HEADER, REFS, synthetic_records(seed, **kw), block_bytes=3000)
    return path


def short_records(n=120000, no_rg_at=None, step=5):
    """`n` short records of one library, so close together that the 100 000-record prevalence stop falls inside a segment
    (step = 1 and 12 000 records: one 16-kbp window, a segment longer than the smallest round)"""
    recs = []
    for i in range(n):
        tags = [] if i == no_rg_at else [("RG", "Z", "r0")]
        recs.append({"name": "s", "flag": QUALIFYING, "tid": 0, "pos": 1000 + step * i, "mapq": 9, "cigar": "10M", "mtid": 0,
                     "mpos": 1200 + 5 * i, "tlen": 200 + i % 7, "tags": tags})
    return recs


def write_short(path, **kw):
    bamwriter.write_bam(path, HEADER, REFS, short_records(**kw), block_bytes=60000)
    return path


def corrupt_member(src, dst):
    """a copy of `src` (and its index) with the payload of a BGZF member in the middle of the file overwritten"""
    data = bytearray(open(src, "rb").read())
    offs, at = [], 0
    while at + 18 <= len(data):
        offs.append(at)
        at += (data[at + 16] | (data[at + 17] << 8)) + 1
    at = offs[len(offs) // 2]
    for i in range(at + 30, at + 30 + 64):
        data[i] = 0xA5
    open(dst, "wb").write(bytes(data))
    shutil.copy(src + ".bai", dst + ".bai")
    return dst


def outcome(fn):
    from svtyper_amd import hip
    try:
        return ("ok", fn())
    except hip.SvtyperHipError as e:
        return ("error", str(e))


def host_scan(bam, groups, num_samp):
    out = []
    for g in groups:
        read_length, hist, in_lib, total = bam.scan_library(g, num_samp)
        out.append((read_length, list(hist.items()), in_lib, total))
    return out


def compare(bam, groups, num_samp, round_bytes=0, route="walk_host", inflate="device", expect_reason=None):
    """the walk against the host scan, library by library; returns the walk's stats"""
    want = outcome(lambda: host_scan(bam, groups, num_samp))
    got = outcome(lambda: bam.scan_libraries(groups, num_samp, route=route, inflate=inflate, round_bytes=round_bytes, ordered=True))
    stats = bam.library_scan_stats
    assert got == want, (num_samp, round_bytes, route, inflate, stats, str(got)[:300], str(want)[:300])
    if expect_reason == WALK:
        assert stats["host_reason"] is None, stats
    elif expect_reason is not None:
        assert stats["host_reason"] == expect_reason, stats
    if want[0] == "error":
        assert stats["host_reason"] is not None, stats       # an error is always the host scan's own
    return stats

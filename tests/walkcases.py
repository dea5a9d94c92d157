"""Inputs shared by tests/test_evidence_walk_host.py (CPU) and tests/test_device_reader.py (GPU): the units of a BAM as the arrays
the reader entries take, the list of BAMs both files compare on, and the units built to leave the envelope of the walk."""
import json
import os

import numpy as np

import goldenio as gio
from svtyper_amd import bam, geometry as geo, library, native_reads as nr, pipeline

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "data")
FIXTURE_BAM = os.path.join(DATA, "NA12878.target_loci.sorted.bam")
SYNTHETIC_SEEDS = (11, 12, 13, 14, 15, 16, 21, 22)


def unit_arrays(sites, sample, nbam, mode):
    """(windows, breakpoints, read groups, library of each read group, flank of each library) of `sites`"""
    tid_of = nbam.gettid
    bps = np.concatenate([geo.breakpoint_record(s["breakpoint"], tid_of) for s in sites])
    win = np.zeros(len(sites), nr.FETCH_DTYPE)
    for k, s in enumerate(sites):
        bp = s["breakpoint"]
        for side, (t, lo, hi) in (("A", ("tid_a", "lo_a", "hi_a")), ("B", ("tid_b", "lo_b", "hi_b"))):
            chrom, a, b = pipeline.fetch_window(sample, bp[side]["chrom"], bp[side]["pos"], bp[side]["ci"],
                                                as_int=(mode == nr.COUNT_SSO))
            win[t][k], win[lo][k], win[hi][k] = tid_of(chrom), int(a), int(b)
    rgs = list(sample.rg_to_lib.keys())
    libs = list(sample.lib_dict.values())
    rg_lib = [libs.index(sample.rg_to_lib[rg]) if sample.rg_to_lib[rg].name in sample.active_libs else -1 for rg in rgs]
    flank = [float(lib.mean) + float(lib.sd) * 3 for lib in libs]
    return win, bps, rgs, rg_lib, flank


def open_sample(path, info):
    sample = library.Sample.from_lib_info(bam.AlignmentFile(path), info, 1e-3)
    return sample, nr.NativeBam(path)


def fixture_input():
    """the reference's BAM x the windows of tests/data/example.vcf"""
    sites = gio.load("fixture_sites.json.gz")["sites"]
    info = json.load(open(os.path.join(DATA, "NA12878.bam.json")))
    sample, nbam = open_sample(FIXTURE_BAM, info)
    return sites, sample, nbam


def synthetic_input(tmp_path, seed, **kw):
    """the random BAMs of tests/soak_geometry.py (test_native_reads._synthetic_bam)"""
    import test_native_reads as N
    path = str(tmp_path / ("syn%d.bam" % seed))
    sites, info = N._synthetic_bam(path, seed, **kw)
    sample, nbam = open_sample(path, info)
    return sites, sample, nbam


def fake_inputs(tmp_path):
    """the fake reads of tests/fakereads.py as the golden carries them (tests/golden/fake_sites.json.gz), one BAM per library
    group written by tests/bamwriter.py: (sites, sample, nbam) per group"""
    import bamwriter as bw
    g = gio.load("fake_sites.json.gz")
    refs = [("1", 400_000), ("2", 400_000)]
    tid_of = {"1": 0, "2": 1}
    for k, group in enumerate(g["groups"]):
        libs = group["libraries"]
        header = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:400000\n@SQ\tSN:2\tLN:400000\n" + "".join(
            "@RG\tID:%s\tSM:fake\tLB:%s\n" % (rg, L["name"]) for L in libs for rg in L["readgroups"])
        recs = []
        for site in group["sites"]:
            for (name, flag, ref, start, cigar, mapq, sa, rg, _qlen, tlen) in site["reads"]:
                tags = [("RG", "Z", rg)] + ([("SA", "Z", sa)] if sa else [])
                recs.append(dict(name=name, flag=flag, tid=tid_of[ref], pos=start, mapq=mapq, cigar=cigar, mtid=tid_of[ref],
                                 mpos=start, tlen=tlen, tags=tags))
        recs.sort(key=lambda r: (r["tid"], r["pos"]))
        path = str(tmp_path / ("fake%d.bam" % k))
        bw.write_bam(path, header, refs, recs, block_bytes=2000 + 500 * k)
        as_float = lambda x: float.fromhex(x) if isinstance(x, str) else float(x)
        info = {"fake": {"mapped": len(recs), "unmapped": 0, "bam": path, "sample_name": "fake", "libraryArray": [
            {"library_name": L["name"], "readgroups": L["readgroups"], "read_length": L["read_length"], "histogram": L["hist"],
             "mean": as_float(L["mean"]), "sd": as_float(L["sd"]), "prevalence": 1.0 / len(libs)} for L in libs]}}
        sample, nbam = open_sample(path, info)
        yield [{"breakpoint": site["breakpoint"]} for site in group["sites"]], sample, nbam


def three_bam_inputs(tmp_path):
    """the three BAMs behind tests/golden/three*.gt.vcf.gz (test_multisample_qual.three_sample_case) with the sites of their VCF"""
    import test_multisample_qual as M
    import test_native_reads as N
    bams, _vcf, lib_json = M.three_sample_case(str(tmp_path))
    info = json.load(open(lib_json))
    sites, _ = N._synthetic_bam(str(tmp_path / "sites_only.bam"), seed=71, n_pairs=8)
    for path in bams.split(","):
        name = os.path.basename(path)[:-4]
        sample, nbam = open_sample(path, {name: info[name]})
        yield sites, sample, nbam


def boundary_input(tmp_path, n_reads):
    """one site whose first window holds exactly `n_reads` countable, kept reads (distinct names) and nothing else"""
    records = [_read("b%04d" % k, 50_000 + k % 40) for k in range(n_reads)]
    sample, nbam = open_sample(write_case(tmp_path, "boundary%d" % n_reads, records), INFO)
    return [{"breakpoint": SITE}], sample, nbam


def truncated_input(tmp_path):
    """a BAM whose last data block is cut in the middle of its last record (the index still points into it)"""
    import zlib
    import bamwriter as bw
    path = write_case(tmp_path, "whole", [_read("ok%d" % k, 50_000 + k) for k in range(6)])
    raw = bytearray(open(path, "rb").read())
    eof = len(bw.bgzf_block(b""))
    blocks, at = [], 0
    while at < len(raw):
        size = (raw[at + 16] | raw[at + 17] << 8) + 1
        blocks.append((at, size))
        at += size
    last_at, last_size = blocks[-2]
    payload = zlib.decompress(bytes(raw[last_at + 18:last_at + last_size - 8]), -15)
    cut = str(tmp_path / "cut.bam")
    with open(cut, "wb") as f:
        f.write(raw[:last_at] + bw.bgzf_block(payload[:-40]) + raw[len(raw) - eof:])
    os.replace(path + ".bai", cut + ".bai")
    sample, nbam = open_sample(cut, INFO)
    return [{"breakpoint": SITE}], sample, nbam


# ---- one site with a few plain reads, and per case the read(s) that take its unit out of the envelope ----------------------
HEADER = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:100000\n@SQ\tSN:2\tLN:100000\n@RG\tID:rg\tSM:s\tLB:lib\n"
SITE = {"id": "d", "svtype": "DEL", "var_length": 800, "A": {"chrom": "1", "pos": 50_050, "ci": [0, 0], "is_reverse": False},
        "B": {"chrom": "1", "pos": 50_851, "ci": [0, 0], "is_reverse": True}}
INFO = {"s": {"mapped": 4, "unmapped": 0, "bam": "x", "sample_name": "s", "libraryArray": [
    {"library_name": "lib", "readgroups": ["rg"], "read_length": 100, "histogram": {str(k): 10 for k in range(200, 500)},
     "mean": 350.0, "sd": 50.0, "prevalence": 1.0}]}}


def _read(name, pos, cigar="100M", tags=None, flag=0x1 | 0x40, mapq=60):
    return dict(name=name, flag=flag, tid=0, pos=pos, mapq=mapq, cigar=cigar, mtid=0, mpos=50_300, tlen=400,
                tags=[("RG", "Z", "rg")] if tags is None else tags)


def envelope_cases(capacity):
    """name -> (records, expected reason, does the host reader fail on it): one case per capacity / malformation"""
    rg = ("RG", "Z", "rg")
    base = [_read("ok%d" % k, 50_000 + k) for k in range(3)]
    many_ops = "".join("1M1I" for _ in range(capacity["cigar"] // 2 + 1)) + "10M"
    sa_entries = "".join("1,%d,+,40S60M,60,0;" % (52_001 + k) for k in range(capacity["sa_entries"] + 1))
    return {
        "reads": ([_read("r%05d" % k, 50_000 + k % 90) for k in range(capacity["reads"] + 1)], "reads", False),
        "name": (base + [_read("n" * (capacity["name"] + 1), 50_010)], "name", False),
        "cigar": (base + [_read("c", 50_010, cigar=many_ops)], "cigar", False),
        "sa_entries": (base + [_read("s", 50_010, cigar="60M40S", tags=[rg, ("SA", "Z", sa_entries)])], "sa_cap", False),
        "no_rg": (base + [_read("g", 50_010, tags=[("NM", "C", 1)])], "no_rg", True),
        "unknown_rg": (base + [_read("u", 50_010, tags=[("RG", "Z", "other")])], "unknown_rg", True),
        "malformed_sa": (base + [_read("m", 50_010, cigar="60M40S", tags=[rg, ("SA", "Z", "1,52001,+,40S60Q,60,0;")])], "malformed", True),
    }


def write_case(tmp_path, name, records):
    """the case's BAM, its records sorted by position"""
    import bamwriter as bw
    path = str(tmp_path / (name + ".bam"))
    bw.write_bam(path, HEADER, [("1", 100000), ("2", 100000)], sorted(records, key=lambda r: r["pos"]))
    return path


def header_batch(sample, bps, split_weight=1.0, disc_weight=1.0):
    """the unit headers and library tables of the units (what the drivers' collector writes), without records"""
    from svtyper_amd import evidence as ev
    n = len(bps)
    units = np.zeros(n, ev.UNIT_DTYPE)
    units["var_length"] = np.where(bps["svtype"] == ev.SVTYPE_CODE["DEL"], bps["var_length"], 0)
    units["pos_delta"] = np.clip(bps["pos_b"].astype(np.int64) - bps["pos_a"].astype(np.int64), -2**31, 2**31 - 1)
    units["svtype"] = bps["svtype"]
    tables = [lib.table() for lib in sample.lib_dict.values()]
    return ev.EvidenceBatch(np.zeros(n + 1, np.uint64), units, np.zeros(0, ev.RECORD_DTYPE), tables, split_weight, disc_weight)

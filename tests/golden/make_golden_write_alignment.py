#!/usr/bin/env python
"""Generate tests/golden/write_alignment.json.gz by running the REFERENCE's own `svtyper -w` code (dev container only).

    python tests/golden/make_golden_write_alignment.py

The reference's classic.sv_genotype(..., alignment_outpath=...) runs through refload with a stand-in `pysam` whose
AlignmentFile(path, 'wb', template) RECORDS what it is handed instead of writing a file -- the project's BAM writer, the code
under test, takes no part --, and whose reads come from the project's reader as a subclass that takes `query_sequence = None`
(svtyper/utils.py:14).  Per write: [query_name, flag, reference_id, reference_start, XV or null]; beside it the read's MAPQ.

Cases (tests/verdictcases.py: golden_cases):
  a      the fixture BAM x tests/data/example.vcf                     VCF == tests/data/example.gt.vcf
  twice  the fixture BAM given twice, --sum_quals                     VCF == example.twice.sumquals.gt.vcf.gz; the second sample
                                                                     adds no read: the (name, flag) set is the run's
  three  three_sample_case of tests/test_multisample_qual.py          VCF == three.gt.vcf.gz; a blank sample in the middle
A case whose lists equal an earlier case's is stored as {"same_as": that case}.
"""
from __future__ import annotations

import gzip
import io
import json
import os
import struct
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refload  # noqa: E402
from svtyper_amd import bam as bam_module  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
BAM = os.path.join(DATA, "NA12878.target_loci.sorted.bam")
VCF = os.path.join(DATA, "example.vcf")
LIBJSON = os.path.join(DATA, "NA12878.bam.json")


class Segment(bam_module.AlignedSegment):
    """a read the reference may set `query_sequence = None` on"""
    __slots__ = ("query_sequence",)


class Reader(bam_module.AlignmentFile):
    def _next_record(self):
        szb = self._bgzf.read(4)
        if len(szb) < 4:
            return None
        size = struct.unpack("<i", szb)[0]
        data = self._bgzf.read(size)
        if len(data) < size:
            return None
        return Segment(self, data)


class Recorder:
    """pysam.AlignmentFile(path, 'wb', template): what write() is handed, in order"""
    opened = []

    def __init__(self, path, template):
        self.path, self.template = path, template.filename
        self.writes, self.mapq = [], []
        self.closed = False
        Recorder.opened.append(self)

    def write(self, read):
        assert read.query_sequence is None          # utils.py:14
        self.writes.append([read.query_name, read.flag, read.reference_id, read.reference_start,
                            read.get_tag("XV") if read.has_tag("XV") else None])
        self.mapq.append(read.mapping_quality)

    def close(self):
        self.closed = True


def alignment_file(path, mode="rb", template=None, **kw):
    if mode == "wb":
        return Recorder(path, template)
    return Reader(path, mode, **kw)


def run(ref, bams, vcf_path, lib_json, sum_quals):
    """(vcf lines without ##fileDate, Recorder) of one reference run with -w"""
    out = io.StringIO()
    out.close = lambda: None
    del Recorder.opened[:]
    with open(vcf_path) as fin:
        ref.classic.sv_genotype(bams, fin, out, 20, 1, 1, 1000000, lib_json, False, "recorded.bam", None, sum_quals, None, 1e10)
    (rec,) = Recorder.opened
    assert rec.closed and rec.template == bams.split(",")[0]
    return [l for l in out.getvalue().split("\n") if not l.startswith("##fileDate=")], rec


def case_of(rec):
    keys = [(w[0], w[1]) for w in rec.writes]
    assert len(set(keys)) == len(keys)              # no (name, flag) is written twice
    return {"writes": rec.writes, "mapq": rec.mapq}


def main():
    pysam = types.ModuleType("pysam")
    pysam.AlignmentFile = alignment_file
    ref = refload.load_reference(pysam_module=pysam)
    cases = {}

    vcf, rec = run(ref, BAM, VCF, LIBJSON, False)
    assert vcf == [l for l in open(os.path.join(DATA, "example.gt.vcf")).read().split("\n") if not l.startswith("##fileDate=")]
    tags = [w[4] for w in rec.writes]
    counts = (len(tags), tags.count("R"), tags.count("A"), tags.count(None))
    assert counts == (42799, 32977, 8065, 1757), counts
    cases["a"] = case_of(rec)

    vcf, rec = run(ref, BAM + "," + BAM, VCF, LIBJSON, True)
    assert vcf == gzip.open(os.path.join(HERE, "example.twice.sumquals.gt.vcf.gz"), "rt").read().split("\n")
    cases["twice"] = case_of(rec)

    from test_multisample_qual import three_sample_case
    with tempfile.TemporaryDirectory() as wd:
        bams, vcf_path, lib_json = three_sample_case(wd)
        vcf, rec = run(ref, bams, vcf_path, lib_json, False)
    assert vcf == gzip.open(os.path.join(HERE, "three.gt.vcf.gz"), "rt").read().split("\n")
    cases["three"] = case_of(rec)

    names = list(cases)
    for i, name in enumerate(names):                 # equal lists are stored once
        for earlier in names[:i]:
            if "same_as" not in cases[earlier] and cases[earlier] == cases[name]:
                cases[name] = {"same_as": earlier}
                break
    path = os.path.join(HERE, "write_alignment.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(cases, separators=(",", ":"), sort_keys=True).encode())
    print("wrote %s (%d bytes)" % (os.path.basename(path), os.path.getsize(path)))
    for name, c in cases.items():
        print(name, c.get("same_as") or "%d writes" % len(c["writes"]))


if __name__ == "__main__":
    main()

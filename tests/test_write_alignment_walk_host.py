"""`svtyper -w` from the walk's source rows, with no GPU: svt_bam_evidence_dump_walk_host (svt_evidence_walk.h with source rows +
svt_dump_rules.h on one lane) against the reference's own -w output (tests/golden/write_alignment.json.gz) and against the BAM
the Python route writes -- record for record, tag for tag and byte for byte.

The verdict bytes the dump takes are verdictcases.restate over the walk's own records (there is no host implementation of the
verdicts in the library); the run-wide (query_name, flag) set is driver.tag_and_write's.  The GPU side of the same comparison is
tests/test_write_alignment_device_reader.py."""
import gzip
import os
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_host_pipeline as T  # noqa: E402
import test_write_alignment_host as W  # noqa: E402
import verdictcases as V  # noqa: E402
from svtyper_amd import bam, driver, evidence as ev, native_reads as nr, pipeline  # noqa: E402
from svtyper_amd.bulk_vcf import SiteArrays  # noqa: E402


def payload(path):
    """the inflated record payload of a BAM: everything behind its header"""
    data = open(path, "rb").read()
    out, at = [], 0
    while at < len(data):
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(zlib.decompress(data[at + 18:at + size - 8], -15))
        at += size
    f = bam.AlignmentFile(path, "rb")
    n_header = len(f._header_bytes)
    f.close()
    return b"".join(out)[n_header:]


def python_route(monkeypatch, bams, vcf_path, lib_json, out_bam, **kw):
    """The Python route's -w run; returns (VCF lines, the run's samples, the breakpoints of its sites in output order)."""
    seen = {"samples": None, "sites": []}
    add = pipeline.UnitCollector.add

    def recording(self, breakpoint, sample_index, fragments, skip=False):
        seen["samples"] = self.samples
        if sample_index == 0:
            seen["sites"].append(breakpoint)
        return add(self, breakpoint, sample_index, fragments, skip=skip)
    monkeypatch.setattr(pipeline.UnitCollector, "add", recording)
    vcf = W.run_w(bams, vcf_path, lib_json, out_bam, **kw)
    monkeypatch.setattr(pipeline.UnitCollector, "add", add)
    return vcf, seen["samples"], seen["sites"]


def sample_calls(samples, paths, sites, max_reads=None):
    """per sample what the device route hands its reader for `sites` (pipeline.NativeUnitCollector, geometry="walk"):
    (NativeBam, the reader entries' arguments, a function from (rec_offset, records, skipped) to the sample's EvidenceBatch)"""
    nbams = [nr.NativeBam(p) for p in paths]
    col = pipeline.NativeUnitCollector(samples, nbams, 1, 1, 20, nr.COUNT_CLASSIC, max_reads, geometry="walk")
    prepared = col._prepare(SiteArrays.from_dicts(sites))
    out = []
    for k, (nbam, (bps, win)) in enumerate(zip(nbams, prepared)):
        rgs, idx = col.rg_tables[k]
        args = (win, bps, rgs, idx, max_reads, nr.COUNT_CLASSIC, col._flanks(k), 20, pipeline.SPLIT_SLOP)

        def batch(off, recs, skipped, k=k, bps=bps):
            units = col._unit_headers(k, bps)
            units["flags"] = np.where(np.asarray(skipped) != 0, ev.UNIT_SKIP, 0)
            return ev.EvidenceBatch(off, units, recs, col.group_tables[col.group_of[k]], 1, 1)
        out.append((nbam, args, batch))
    return out


def host_dump(samples, paths, sites, max_reads=None):
    """evidence_dump_walk_host per sample over `sites`; the units' evidence site-major and sample-minor, as
    pipeline.NativeUnitCollector(keep_reads=True) hands it to driver.tag_and_write, and the counters summed"""
    n_samp, evidence, total = len(samples), [None] * (len(sites) * len(samples)), {}
    for k, (nbam, args, batch) in enumerate(sample_calls(samples, paths, sites, max_reads)):
        off, recs, skipped, flagged, _kept = nbam.evidence_walk_host(*args)
        data, unit_off, unit_host, counters = nbam.evidence_dump_walk_host(*args, V.restate(batch(off, recs, skipped)))
        assert unit_host.tolist() == (flagged != 0).astype(int).tolist()      # nothing of these inputs leaves the dump's own envelope
        assert len(data) == unit_off[-1] == counters["n_bytes"]
        for key, v in counters.items():
            total[key] = total.get(key, 0) + v
        for i in range(len(sites)):
            if not skipped[i]:
                assert not unit_host[i]
                evidence[i * n_samp + k] = memoryview(data)[int(unit_off[i]):int(unit_off[i + 1])]
    return evidence, total


def write_dump(path, template_path, evidence, chunk=None):
    template = bam.AlignmentFile(template_path, "rb")
    out = bam.AlignmentFile(path, "wb", template=template)
    template.close()
    written = set()
    step = chunk or max(len(evidence), 1)
    for at in range(0, len(evidence), step):                       # (the set holds across the chunks of a run)
        driver.tag_and_write(evidence[at:at + step], out, written)
    out.close()


@pytest.fixture(scope="module")
def golden():
    return V.golden_cases()


def test_fixture_case_a(tmp_path, golden, monkeypatch):
    want_bam, got_bam = str(tmp_path / "python.bam"), str(tmp_path / "walk.bam")
    vcf, samples, sites = python_route(monkeypatch, T.IN_BAM, T.IN_VCF, T.LIB_JSON, want_bam)
    assert vcf == W.no_date(open(T.EXPECTED).read()) and len(sites) > 200
    evidence, counters = host_dump(samples, [T.IN_BAM], sites)
    write_dump(got_bam, T.IN_BAM, evidence)
    W.same_writes(got_bam, golden["a"])
    tags = [w[4] for w in V.written_records(got_bam)[0]]
    assert (len(tags), tags.count("R"), tags.count("A"), tags.count(None)) == (42799, 32977, 8065, 1757)
    assert payload(got_bam) == payload(want_bam)
    # the dump itself holds a read once per unit that writes it: more records than the run-wide set lets through
    assert counters["n_reads"] >= len(tags) and counters["units_host"] == 0 and counters["units_dumped"] > 100


def test_fixture_twice(tmp_path, golden, monkeypatch):
    want_bam, got_bam = str(tmp_path / "python.bam"), str(tmp_path / "walk.bam")
    vcf, samples, sites = python_route(monkeypatch, T.IN_BAM + "," + T.IN_BAM, T.IN_VCF, T.LIB_JSON, want_bam, sum_quals=True)
    assert vcf == gzip.open(os.path.join(HERE, "golden", "example.twice.sumquals.gt.vcf.gz"), "rt").read().split("\n")
    assert len(samples) == 2
    evidence, _counters = host_dump(samples, [T.IN_BAM, T.IN_BAM], sites)
    write_dump(got_bam, T.IN_BAM, evidence)
    W.same_writes(got_bam, golden["twice"])
    assert payload(got_bam) == payload(want_bam)


@pytest.mark.parametrize("chunk", [None, 7])
def test_three_samples(tmp_path, golden, monkeypatch, chunk):
    from test_multisample_qual import three_sample_case
    bams, vcf_path, lib_json = three_sample_case(str(tmp_path))
    want_bam, got_bam = str(tmp_path / "python.bam"), str(tmp_path / "walk.bam")
    _vcf, samples, sites = python_route(monkeypatch, bams, vcf_path, lib_json, want_bam)
    paths = bams.split(",")
    assert len(samples) == len(paths) == 3
    evidence, _counters = host_dump(samples, paths, sites)
    write_dump(got_bam, paths[0], evidence, chunk=chunk)
    W.same_writes(got_bam, golden["three"])
    assert payload(got_bam) == payload(want_bam)


def test_a_skipped_unit_has_no_bytes(monkeypatch, tmp_path):
    """--max_reads 300 skips variant 99771 of the fixture: its unit is None for tag_and_write, its slice of the dump is empty"""
    _vcf, samples, sites = python_route(monkeypatch, T.IN_BAM, T.IN_VCF, T.LIB_JSON, str(tmp_path / "python.bam"), max_reads=300)
    evidence, _counters = host_dump(samples, [T.IN_BAM], sites, max_reads=300)
    assert sum(e is None for e in evidence) == 1


def test_verdicts_have_to_match_the_records():
    nbam = nr.NativeBam(T.IN_BAM)
    with pytest.raises(Exception, match="one verdict byte per record"):
        import walkcases as WC
        sites, sample, nb = WC.fixture_input()
        win, bps, rgs, rg_lib, flank = WC.unit_arrays(sites[:5], sample, nb, nr.COUNT_CLASSIC)
        nbam.evidence_dump_walk_host(win, bps, rgs, rg_lib, None, nr.COUNT_CLASSIC, flank, 20, 3, np.zeros(3, np.uint8))


def test_write_raw_takes_whole_records_only(tmp_path):
    src = bam.AlignmentFile(T.IN_BAM, "rb")
    out = bam.AlignmentFile(str(tmp_path / "raw.bam"), "wb", template=src)
    src.close()
    with pytest.raises(ValueError, match="one whole record"):
        out.write_raw(struct.pack("<i", 40) + b"\0" * 39)
    out.close()

"""The edge corpus of the evidence dump (tests/dumpcases.py) with no GPU: what the corpus reaches, asserted from the Python route's
output alone, and svt_bam_evidence_dump_walk_host against that output byte for byte -- the LDS tier, the deep tier of the walk,
and a unit outside the walk's envelope, which comes back flagged and without bytes."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import dumpcases as D  # noqa: E402
import test_write_alignment_host as W  # noqa: E402
import test_write_alignment_walk_host as H  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def python_bam(monkeypatch, tmp_path, **kw):
    path, vcf, lib_json = D.write_case(tmp_path, **kw)
    want_bam = str(tmp_path / "python.bam")
    _vcf, samples, sites = H.python_route(monkeypatch, path, vcf, lib_json, want_bam)
    assert [s["id"] for s in sites] == [ident for _a, ident in D.SITES]
    return path, want_bam, samples, sites


def test_the_corpus_reaches_what_it_is_for(monkeypatch, tmp_path):
    _path, want_bam, _samples, sites = python_bam(monkeypatch, tmp_path)
    f, written = W.all_records(want_bam)
    f.close()
    by_name = D.reach(written, D.records())
    assert (sites[1]["A"]["pos"], sites[1]["B"]["pos"]) == (D.A0, D.B0)
    # empty first and last units: nothing of the corpus lies in their windows, the two in the middle write
    assert {n[:5] for n in by_name if n.startswith("small")} == {"small"} and "t00" in by_name
    # a record's end on both sides of a 64-byte step of the output, and every destination alignment mod 4
    ends, at = set(), 0
    for r in written:
        at += 4 + len(r._raw)                           # (block_size and the record, as it lies in the output)
        ends.add(at % 64)
    print(sorted(ends))
    assert {e % 4 for e in ends} == {0, 1, 2, 3} and ends & {61, 62, 63} and ends & {1, 2, 3}


@pytest.mark.parametrize("deep", [False, True])
def test_host_dump_is_the_python_route(monkeypatch, tmp_path, deep):
    path, want_bam, samples, sites = python_bam(monkeypatch, tmp_path, deep=deep)
    evidence, counters = H.host_dump(samples, [path], sites)
    assert counters["units_dumped"] == 2 and counters["units_host"] == 0 and counters["n_reads"] > 150
    assert len(evidence[0]) == 0 and len(evidence[3]) == 0 and len(evidence[1]) > len(evidence[2]) > 0
    got_bam = str(tmp_path / "walk.bam")
    H.write_dump(got_bam, path, evidence)
    assert H.payload(got_bam) == H.payload(want_bam)
    if deep:
        nbam = nr.NativeBam(path)
        import walkcases as WC
        a = WC.unit_arrays([{"breakpoint": s} for s in sites], samples[0], nbam, nr.COUNT_CLASSIC)
        kept = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_CLASSIC, a[4], 20, 3)[4]
        assert kept[1] > nr.walk_capacities()["reads_lds"]          # the main unit took the deep tier


def test_a_unit_outside_the_envelope_comes_back_flagged(monkeypatch, tmp_path):
    """a 129-byte query name: the unit is outside the walk's envelope, so the dump holds nothing of it and says so"""
    import numpy as np
    import verdictcases as V
    from svtyper_amd import evidence as ev, pipeline
    from svtyper_amd.bulk_vcf import SiteArrays
    path, _want_bam, samples, sites = python_bam(monkeypatch, tmp_path, long_name=True)
    nbam = nr.NativeBam(path)
    col = pipeline.NativeUnitCollector(samples, [nbam], 1, 1, 20, nr.COUNT_CLASSIC, None, geometry="walk")
    (bps, win), = col._prepare(SiteArrays.from_dicts(sites))
    rgs, idx = col.rg_tables[0]
    args = (win, bps, rgs, idx, None, nr.COUNT_CLASSIC, col._flanks(0), 20, pipeline.SPLIT_SLOP)
    off, recs, skipped, flagged, _kept = nbam.evidence_walk_host(*args)
    assert flagged.tolist() == [0, 0, 4, 0]
    units = col._unit_headers(0, bps)
    batch = ev.EvidenceBatch(off, units, recs, col.group_tables[0], 1, 1)
    data, unit_off, unit_host, counters = nbam.evidence_dump_walk_host(*args, V.restate(batch))
    assert unit_host.tolist() == [0, 0, 1, 0] and unit_off[2] == unit_off[3] == len(data) > 0
    assert counters["units_host"] == 1 and counters["units_outside_dump"] == 0 and counters["units_dumped"] == 1

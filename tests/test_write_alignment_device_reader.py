"""GPU: `svtyper -w` with the device reader -- classic.sv_genotype(..., alignment_outpath, reader="device"), the evidence reads
built on the GPU by svt_dump_kernel.h behind svt_verdict_kernel -- against the reference's own -w output
(tests/golden/write_alignment.json.gz) and the BAM the Python route writes, byte for byte; the dump of
svt_bam_evidence_device_dump against svt_bam_evidence_dump_walk_host over the edge corpus (tests/dumpcases.py), the deep tier and
a unit the host reader recomputes included; and the device reader without the dump, which is what it was.
(tests/test_write_alignment_walk_host.py and tests/test_write_alignment_dump_corpus.py are the CPU side.)"""
import gzip
import io
import os

import numpy as np
import pytest

import dumpcases as D
import test_host_pipeline as T
import test_write_alignment_host as W
import test_write_alignment_walk_host as H
import verdictcases as V
from svtyper_amd import bam, classic, driver, native_reads as nr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def run_w(bams, vcf_path, lib_json, out_bam, sum_quals=False, engine=None, **kw):
    """sv_genotype with -w and reader="device" (engine=None: the HIP engine); returns the VCF lines without ##fileDate"""
    out = io.StringIO()
    out.close = lambda: None
    with open(vcf_path) as inf:
        classic.sv_genotype(bams, inf, out, 20, 1, 1, 1000000, lib_json, False, out_bam, None, sum_quals, None, 1e10, engine=engine,
                            reader="device", **kw)
    return W.no_date(out.getvalue())


@pytest.fixture(scope="module")
def python_a(tmp_path_factory):
    """case `a` through the Python route (the oracle engine: no device in the yardstick): its BAM, samples and sites"""
    mp = pytest.MonkeyPatch()
    out_bam = str(tmp_path_factory.mktemp("python_a") / "python.bam")
    _vcf, samples, sites = H.python_route(mp, T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam)
    mp.undo()
    return out_bam, samples, sites


@pytest.fixture(scope="module")
def python_three(tmp_path_factory):
    from test_multisample_qual import three_sample_case
    tmp = tmp_path_factory.mktemp("python_three")
    bams, vcf_path, lib_json = three_sample_case(str(tmp))
    out_bam = str(tmp / "python.bam")
    W.run_w(bams, vcf_path, lib_json, out_bam)
    return bams, vcf_path, lib_json, out_bam


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_fixture_case_a(tmp_path, hip_device, python_a, inflate):
    out_bam = str(tmp_path / "a.bam")
    stats = {}
    vcf = run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam, inflate=inflate, stats=stats)
    assert vcf == W.no_date(open(T.EXPECTED).read())
    W.same_writes(out_bam, V.golden_cases()["a"])
    assert H.payload(out_bam) == H.payload(python_a[0])
    f, t = bam.AlignmentFile(out_bam, "rb"), bam.AlignmentFile(T.IN_BAM, "rb")
    assert f._header_bytes == t._header_bytes                       # the first -B file is the template
    f.close()
    t.close()
    d = stats["device_reader"]
    print(d["dump"], stats["route"])
    assert stats["route"] == "per line" and d["units_host"] == 0
    assert d["dump"]["units_host"] == 0 and d["dump"]["n_reads"] >= 42799 and d["dump"]["units_dumped"] > 100


def test_fixture_twice(tmp_path, hip_device):
    out_bam = str(tmp_path / "twice.bam")
    vcf = run_w(T.IN_BAM + "," + T.IN_BAM, T.IN_VCF, T.LIB_JSON, out_bam, sum_quals=True)
    assert vcf == gzip.open(os.path.join(HERE, "golden", "example.twice.sumquals.gt.vcf.gz"), "rt").read().split("\n")
    W.same_writes(out_bam, V.golden_cases()["twice"])


@pytest.mark.parametrize("chunk", [None, 7])
def test_three_samples(tmp_path, hip_device, python_three, monkeypatch, chunk):
    from svtyper_amd.pipeline import HipEngine
    bams, vcf_path, lib_json, want_bam = python_three
    if chunk:
        monkeypatch.setattr(driver, "WRITE_CHUNK_UNITS", chunk)
    out_bam = str(tmp_path / "three.bam")
    vcf = run_w(bams, vcf_path, lib_json, out_bam, engine=HipEngine(hip_device, verdicts=True))
    assert vcf == gzip.open(os.path.join(HERE, "golden", "three.gt.vcf.gz"), "rt").read().split("\n")
    W.same_writes(out_bam, V.golden_cases()["three"])
    assert H.payload(out_bam) == H.payload(want_bam)


def corpus(tmp_path, **kw):
    path, vcf, lib_json = D.write_case(tmp_path, **kw)
    mp = pytest.MonkeyPatch()
    want_bam = str(tmp_path / "python.bam")
    _vcf, samples, sites = H.python_route(mp, path, vcf, lib_json, want_bam)
    mp.undo()
    return path, vcf, lib_json, want_bam, samples, sites


@pytest.mark.parametrize("deep", [False, True])
@pytest.mark.parametrize("inflate", ["host", "device"])
def test_the_device_dump_is_the_host_dump(tmp_path, hip_device, inflate, deep):
    path, _vcf, _lib_json, _want, samples, sites = corpus(tmp_path, deep=deep)
    (nbam, args, batch), = H.sample_calls(samples, [path], sites)
    off, recs, skipped, flagged, kept = nbam.evidence_walk_host(*args)
    assert not flagged.any() and (kept[1] > nr.walk_capacities()["reads_lds"]) == deep
    want = nbam.evidence_dump_walk_host(*args, V.restate(batch(off, recs, skipped)))
    head = batch(np.zeros(len(sites) + 1, np.uint64), recs[:0], np.zeros(len(sites)))
    got = []
    for _ in range(2):                                              # two calls in one process: the same bytes
        d, _skipped, stats, dump = nbam.evidence_device(*args, head, hip_device, 0, 2, inflate=inflate, dump=True)
        got_off, got_recs = nr.batch_records(d)
        d.close()
        assert np.array_equal(got_off, off) and got_recs.tobytes() == recs.tobytes()
        assert stats["deep"]["units_deep"] == (1 if deep else 0)
        got.append((dump, stats["dump"]))
    for (data, unit_off, unit_host), counters in got:
        assert unit_off.tolist() == want[1].tolist() and unit_host.tolist() == want[2].tolist() == [0, 0, 0, 0]
        assert data == want[0] and len(data) > 10000
        assert {k: v for k, v in counters.items() if k != "dump_s"} == {k: v for k, v in want[3].items() if k != "dump_s"}


@pytest.mark.parametrize("deep", [False, True])
def test_the_corpus_through_the_driver(tmp_path, hip_device, deep):
    path, vcf, lib_json, want_bam, _samples, _sites = corpus(tmp_path, deep=deep)
    out_bam = str(tmp_path / "device.bam")
    run_w(path, vcf, lib_json, out_bam)
    assert H.payload(out_bam) == H.payload(want_bam)


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_a_unit_of_the_host_reader_is_written_by_the_python_reader(tmp_path, hip_device, inflate):
    """a 129-byte query name puts one unit outside the walk's envelope: the host reader recomputes it, the dump holds nothing of
    it, and its reads come from the Python reader with the unit's slice of the batch's verdicts"""
    path, vcf, lib_json, want_bam, _samples, _sites = corpus(tmp_path, long_name=True)
    out_bam = str(tmp_path / "device.bam")
    stats = {}
    run_w(path, vcf, lib_json, out_bam, inflate=inflate, stats=stats)
    d = stats["device_reader"]
    assert d["units_host"] == 1 and d["units_host_by_reason"] == {"name": 1}
    assert d["dump"]["units_host"] == 1 and d["dump"]["units_outside_dump"] == 0 and d["dump"]["units_dumped"] == 1
    assert H.payload(out_bam) == H.payload(want_bam)
    f, written = W.all_records(out_bam)
    f.close()
    assert any(r.query_name == "L" * 129 for r in written)


def test_without_the_dump_the_device_reader_is_what_it_was(hip_device, python_a):
    _bam, samples, sites = python_a
    (nbam, args, batch), = H.sample_calls(samples, [T.IN_BAM], sites[:60])
    head = batch(np.zeros(61, np.uint64), np.zeros(0, V.RECORD_DTYPE), np.zeros(60))
    d, skipped, stats = nbam.evidence_device(*args, head, hip_device, 0, 2)
    plain = nr.batch_records(d)
    d.close()
    assert stats["dump"] == nr.NO_DUMP and all(v == 0 for v in stats["dump"].values())
    d, skipped2, stats2, dump = nbam.evidence_device(*args, head, hip_device, 0, 2, dump=True)
    dumped = nr.batch_records(d)
    verdicts = d.verdicts()
    d.close()
    assert np.array_equal(plain[0], dumped[0]) and plain[1].tobytes() == dumped[1].tobytes() and np.array_equal(skipped, skipped2)
    assert stats2["dump"]["n_reads"] > 0 and stats2["dump"]["n_bytes"] == len(dump[0]) == dump[1][-1]
    # ... and the dump is the host's over the same records with the device's own verdicts
    want = nbam.evidence_dump_walk_host(*args, verdicts)
    assert dump[0] == want[0] and dump[1].tolist() == want[1].tolist()

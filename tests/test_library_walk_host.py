"""The library scans of a whole file in one segmented walk (svtyper_amd/csrc/svt_library_walk.h) on the CPU:
svt_bam_scan_libraries_walk_host -- the walk with one lane, members inflated by svt_inflate.h -- against svt_bam_scan_library per
library.  The same cases run on the GPU in tests/test_library_scan_device.py."""
import io
import os
import shutil

import pytest

import libscancases as lc
from libscancases import WALK

ROOT = lc.ROOT


@pytest.fixture(scope="module")
def native():
    from svtyper_amd import hip, native_reads
    hip.build()
    return native_reads


@pytest.fixture(scope="module")
def fixture_bam(native):
    b = native.NativeBam(lc.FIXTURE)
    yield b
    b.close()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("libscan"))


@pytest.fixture(scope="module")
def synthetic(native, workdir):
    bams = [native.NativeBam(lc.write_synthetic(os.path.join(workdir, "syn%d.bam" % seed), seed)) for seed in (1, 2, 3)]
    yield bams
    for b in bams:
        b.close()


@pytest.fixture(scope="module")
def short_bam(native, workdir):
    b = native.NativeBam(lc.write_short(os.path.join(workdir, "short.bam")))
    yield b
    b.close()


def test_capacities(native):
    cap = native.library_scan_capacities()
    assert cap["libraries"] >= 3 and cap["read_groups"] >= cap["libraries"] and cap["record"] == 65536
    assert 36242 < cap["dense_keys"] <= 1 << 20 and cap["overflow"] >= 1024
    # the tables stay well under the 256 MiB the deep workspace allows itself
    assert 16 * (cap["libraries"] * cap["dense_keys"] + cap["overflow"]) <= 64 << 20
    assert cap["round_bytes"] == 64 << 20


@pytest.mark.parametrize("round_bytes", [0, lc.SMALL_ROUND])
@pytest.mark.parametrize("num_samp", lc.FIXTURE_NUM_SAMP)
def test_fixture(fixture_bam, num_samp, round_bytes):
    groups = [[rg["ID"] for rg in fixture_bam.header["RG"]]]
    st = lc.compare(fixture_bam, groups, num_samp, round_bytes, expect_reason=WALK)
    assert st["rounds"] == (1 if round_bytes == 0 else 19)
    assert st["segments"] >= 260 and st["records_walked"] == 42801 and 4.8e6 < st["inflated_bytes"] < 5.0e6 * (1 if round_bytes == 0 else 1.3)


def test_fixture_facts(fixture_bam):
    (read_length, hist, in_lib, total), = fixture_bam.scan_libraries([["NA12878.S1"]], 0, route="walk_host", ordered=True)
    assert (read_length, in_lib, total) == (101, 42801, 42801)      # the read-length stop (10 001 reads) falls inside the file
    assert sum(c for _, c in hist) == 21277 and len(hist) == 2755 and max(k for k, _ in hist) == 36242


@pytest.mark.parametrize("round_bytes", [0, lc.SMALL_ROUND])
@pytest.mark.parametrize("num_samp", [0, 1, 150, 1000000])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_synthetic(synthetic, which, num_samp, round_bytes):
    st = lc.compare(synthetic[which], lc.GROUPS, num_samp, round_bytes, expect_reason=WALK)
    assert st["segments"] > 20 and st["records_walked"] == 3000          # the unplaced reads (one without RG) are not scanned
    if num_samp == 0:
        assert st["overflow_entries"] == 10                              # the reads of K, K + 1, 300 000 and 2^31 - 1


def test_synthetic_shapes(synthetic):
    """what the synthetic file is there for: B absent from the first half, keys first seen in several segments, keys around K"""
    K = lc.capacities()["dense_keys"]
    res = synthetic[0].scan_libraries(lc.GROUPS, 0, route="walk_host", ordered=True)
    keys = [k for k, _ in res[0][1]] + [k for k, _ in res[1][1]] + [k for k, _ in res[2][1]]
    assert {K - 1, K, K + 1, 300000, 2 ** 31 - 1} <= set(keys) and min(keys) > 0
    assert all(r[3] == 3000 for r in res) and 0 < res[1][2] < res[0][2]
    # one library alone, a group order that is not the header's, a library without read groups
    lc.compare(synthetic[0], [["r4", "r1"]], 0, lc.SMALL_ROUND, expect_reason=WALK)
    lc.compare(synthetic[0], [["r3"], [], ["r2", "r0"]], 40, 0, expect_reason=WALK)


@pytest.mark.parametrize("round_bytes", [0, lc.SMALL_ROUND])
def test_prevalence_stop_inside_a_segment(short_bam, round_bytes):
    st = lc.compare(short_bam, [["r0"], ["r1"]], 1000000, round_bytes, expect_reason=WALK)
    assert st["records_walked"] == 120000
    res = short_bam.scan_libraries([["r0"]], 500, route="walk_host", round_bytes=lc.SMALL_ROUND)
    assert res[0][2:] == (100000, 100000) and sum(res[0][1].values()) == 500
    assert short_bam.library_scan_stats["records_walked"] < 120000       # every stop reached: the later rounds are not taken


def test_segment_longer_than_a_round(native, workdir):
    """12 000 records in one 16-kbp window: the round is the segment's head, cut open, the next one starts where it stopped"""
    b = native.NativeBam(lc.write_short(os.path.join(workdir, "dense.bam"), n=12000, step=1))
    st = lc.compare(b, [["r0"], ["r1"]], 11000, lc.SMALL_ROUND, expect_reason=WALK)
    assert st["rounds"] >= 3 and st["records_walked"] == 12000 and st["segments"] == st["rounds"]
    assert lc.compare(b, [["r0"]], 0, 0, expect_reason=WALK)["rounds"] == 1
    b.close()


# ---- the envelope: a nonzero host_reason, and the host scan's result or error ---------------------------------------------------
def test_record_without_rg_in_front_of_the_stop(native, workdir):
    recs = lc.synthetic_records(5, n=400, unplaced=0)
    recs[37]["tags"] = [("NM", "C", 1)]
    path = os.path.join(workdir, "norg.bam")
    lc.bamwriter.write_bam(path, lc.HEADER, lc.REFS, recs, block_bytes=3000)
    b = native.NativeBam(path)
    for rb in (0, lc.SMALL_ROUND):
        lc.compare(b, lc.GROUPS, 1000000, rb, expect_reason="no_rg")
    with pytest.raises(Exception, match="without a usable RG tag: q00037"):
        b.scan_libraries(lc.GROUPS, 1000000, route="walk_host")
    b.close()


def test_record_without_rg_behind_every_stop(native, workdir):
    """The choice, pinned: a record without RG in a round the walk took sends the call to the host scan even when it lies behind
    every stop (the host scan never gets there and answers without an error); in a round that is not taken it is not seen."""
    b = native.NativeBam(lc.write_short(os.path.join(workdir, "norg_late.bam"), no_rg_at=110000))
    lc.compare(b, [["r0"]], 100, 0, expect_reason="no_rg")
    lc.compare(b, [["r0"]], 100, lc.SMALL_ROUND, expect_reason=WALK)
    b.close()


def test_more_libraries_than_the_tables_hold(synthetic):
    n = lc.capacities()["libraries"] + 1
    lc.compare(synthetic[0], [["r%d" % (k % 6)] if k < 6 else ["x%d" % k] for k in range(n)], 50, 0, expect_reason="tables")
    lc.compare(synthetic[0], [["r0"], ["r0", "r1"]], 50, 0, expect_reason="tables")      # a read group of two libraries


def test_full_overflow_list(native, synthetic):
    native.library_scan_overflow_limit(3)
    try:
        st = lc.compare(synthetic[1], lc.GROUPS, 0, 0, expect_reason="overflow")
        assert st["overflow_entries"] > 3
        lc.compare(synthetic[1], lc.GROUPS, 1, 0, expect_reason=WALK)                    # (nothing beyond K among the first reads)
    finally:
        native.library_scan_overflow_limit(0)
    lc.compare(synthetic[1], lc.GROUPS, 0, 0, expect_reason=WALK)


def test_corrupted_member(native, workdir):
    path = lc.corrupt_member(os.path.join(workdir, "syn1.bam"), os.path.join(workdir, "corrupt.bam"))
    b = native.NativeBam(path)
    for rb in (0, lc.SMALL_ROUND):
        st = lc.compare(b, lc.GROUPS, 0, rb)
        assert st["host_reason"] in ("member", "record"), st
    b.close()


def test_file_without_index(native, workdir):
    """the reader's handle is the walk's only way in, and it needs the index: there is no handle to scan, on either route"""
    path = os.path.join(workdir, "noindex.bam")
    shutil.copy(os.path.join(workdir, "syn1.bam"), path)
    from svtyper_amd import hip
    with pytest.raises(hip.SvtyperHipError, match="no .bai index"):
        native.NativeBam(path)


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_sample_from_bam_through_the_walk_matches_the_reference(native):
    import goldenio as gio
    from svtyper_amd import bam, library
    g = gio.load("library_from_bam.json.gz")
    nb = native.NativeBam(lc.FIXTURE)
    sample = library.Sample.from_bam(bam.AlignmentFile(lc.FIXTURE), 1000000, 1e-3, nb, library_scan="walk_host")
    assert nb.library_scan_stats["host_reason"] is None and nb.library_scan_stats["segments"] >= 260
    assert sample.name == g["sample"] and sample.active_libs == g["active_libs"]
    assert float(sample.get_fetch_flank(3)).hex() == g["fetch_flank_z3"]
    assert len(sample.lib_dict) == len(g["libraries"])
    for lib, want in zip(sample.lib_dict.values(), g["libraries"]):
        assert lib.name == want["name"] and lib.readgroups == want["readgroups"] and lib.read_length == want["read_length"]
        assert float(lib.mean).hex() == want["mean"] and float(lib.sd).hex() == want["sd"]
        assert float(lib.prevalence).hex() == want["prevalence"]
        assert {str(k): int(v) for k, v in lib.hist.items()} == want["hist"]
    # the library file written from it is the host scan's, byte for byte
    texts = []
    for scan in ("host", "walk_host"):
        out = io.StringIO()
        out.close = lambda: None
        library.write_sample_json([library.Sample.from_bam(bam.AlignmentFile(lc.FIXTURE), 1000000, 1e-3, nb, library_scan=scan)], out)
        texts.append(out.getvalue())
    assert texts[0] == texts[1] and len(texts[0]) > 10000
    nb.close()


def test_library_scan_device_needs_the_native_reader():
    from svtyper_amd import classic, singlesample
    bam, vcf = lc.FIXTURE, os.path.join(ROOT, "tests", "data", "example.vcf")
    with open(vcf) as f, pytest.raises(ValueError, match="library_scan"):
        singlesample.sso_genotype(bam, f, io.StringIO(), 20, 1, 1, 1000000, None, False, None, False, 1000, 1e10, None, 1000,
                                  reader="python", library_scan="device")
    with open(vcf) as f, pytest.raises(ValueError, match="library_scan"):
        classic.sv_genotype(bam, f, io.StringIO(), 20, 1, 1, 1000000, None, False, None, None, False, None, 1e10,
                            reader="python", library_scan="device")
    with open(vcf) as f, pytest.raises(ValueError, match="library_scan"):
        singlesample.sso_genotype(bam, f, io.StringIO(), 20, 1, 1, 1000000, None, False, None, False, 1000, 1e10, None, 1000,
                                  reader="native", library_scan="gpu")

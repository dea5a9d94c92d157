"""CSI indexes on every host reader route (svtyper_amd/csrc/svt_bam_index.h behind svt_reads.cpp, svtyper_amd/bam.py): a BAM that
carries only a .csi -- in several binning schemes, written by tests/csiwriter.py -- gives what its BAI-indexed copy gives, and
contigs beyond 2^29 give what the reference made of the same reads (tests/golden/long_contig_sites.json.gz).  CPU only; the
GPU routes are tests/test_csi_index_device.py."""
import io
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import bamwriter as bw
import csicases as CC
import csiwriter
import goldenio as gio
import libscancases as lc
import walkcases as W
from svtyper_amd import bam, classic, evidence as ev, hip, library, native_reads as nr, singlesample

ROOT = lc.ROOT
DATA = os.path.join(ROOT, "tests", "data")
EXAMPLE_VCF = os.path.join(DATA, "example.vcf")
EXPECTED_VCF = os.path.join(DATA, "example.gt.vcf")
LIB_JSON = os.path.join(DATA, "NA12878.bam.json")
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    hip.build()
    return tmp_path_factory.mktemp("csi")


@pytest.fixture(scope="module")
def inputs(workdir):
    """{label: (sites, sample, nbam, shapes)} of the BAI-indexed BAMs (csicases.walk_inputs), made once"""
    return {label: rest for label, *rest in CC.walk_inputs(workdir)}


@pytest.fixture(scope="module")
def copies(workdir, inputs):
    """(label, shape) -> path of the CSI-only copy"""
    made = {}

    def get(label, shape):
        if (label, shape) not in made:
            made[(label, shape)] = CC.csi_only_copy(inputs[label][2].filename, workdir / ("%s_%d_%d" % ((label,) + shape)), shape)
        return made[(label, shape)]
    return get


@pytest.fixture(scope="module")
def long_groups(workdir):
    return CC.long_contig_groups(workdir)


LABELS = ("fixture", "syn11", "syn12", "fake0", "three0", "three1", "three2")


def shapes_of(label):
    return CC.FIXTURE_SHAPES if label == "fixture" else CC.SMALL_SHAPES


CASES = [(label, shape) for label in LABELS for shape in shapes_of(label)]


def linear_records(path):
    """(name, flag, tid, pos, end) of every placed record, by csiwriter's own walk of the inflated file (names by struct)"""
    stream, _blocks, _end = csiwriter.inflate_bam(path)
    _n_ref, recs = csiwriter.records_of(stream)
    out = []
    for s, _e, tid, pos, end, flag in recs:
        l_name = stream[s + 12]
        out.append((stream[s + 36:s + 36 + l_name - 1].decode(), flag, tid, pos, end))
    return out


# ------------------------------------------------------------------------------------------ 1. the loader
def test_a_14_5_csi_holds_what_the_bai_holds(workdir, inputs):
    """bin -> chunks of a bamwriter-made BAM: its .bai against a (14, 5) CSI of the same file, in bam.py.  bamwriter's .bai
    carries no counts, so the CSI's mapped / unmapped are held against a count of the records themselves."""
    n_bins = 0
    for label in LABELS[1:]:
        path = inputs[label][2].filename
        with_bai = bam.AlignmentFile(path)
        with_csi = bam.AlignmentFile(CC.csi_only_copy(path, workdir / ("loader_" + label), (14, 5)))
        assert with_bai.index_info() == {"kind": "bai", "min_shift": 14, "depth": 5}
        assert with_csi.index_info() == {"kind": "csi", "min_shift": 14, "depth": 5}
        assert len(with_csi._index) == len(with_bai._index) == len(with_bai.references)
        for (bins_b, linear, none_b), (bins_c, none_c, loffset) in zip(with_bai._index, with_csi._index):
            assert none_b is None and none_c is None and linear is not None
            assert {b: [tuple(c) for c in v] for b, v in bins_b.items()} == {b: [tuple(c) for c in v] for b, v in bins_c.items()}
            assert set(loffset) == set(bins_c)
            n_bins += len(bins_c)
        recs = linear_records(path)
        assert (with_csi.mapped, with_csi.unmapped) == (sum(1 for r in recs if not r[1] & 4), sum(1 for r in recs if r[1] & 4))
        assert with_csi.mapped > 100
    assert n_bins > 20


def test_fixture_counts_are_the_bais(copies):
    """the fixture's .bai was written by samtools and carries the pseudo-bins: the CSI's counts are its counts"""
    want = bam.AlignmentFile(W.FIXTURE_BAM)
    assert (want.mapped, want.unmapped) == (42801, 0)
    for shape in CC.FIXTURE_SHAPES:
        got = bam.AlignmentFile(copies("fixture", shape))
        assert (got.mapped, got.unmapped) == (want.mapped, want.unmapped)


@pytest.mark.parametrize("label,shape", CASES)
def test_every_shape_reports_itself(copies, label, shape):
    want = {"kind": "csi", "min_shift": shape[0], "depth": shape[1]}
    path = copies(label, shape)
    assert nr.NativeBam(path).index_info() == want and bam.AlignmentFile(path).index_info() == want


def test_aux_bytes_are_skipped(workdir, inputs):
    sites, sample, nbam, _ = inputs["syn12"]
    path = CC.csi_only_copy(nbam.filename, workdir / "aux", (14, 6), aux=b"\x07" * 37, member_bytes=64)
    s2, nb2 = CC.on_copy(sample, path)
    assert nb2.index_info() == s2.bam.index_info() == {"kind": "csi", "min_shift": 14, "depth": 6}
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    want = nbam.evidence(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 1)
    got = nb2.evidence(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)) and len(want[1]) > 100
    assert len(csiwriter.inflate_bam(path + ".csi")[1]) > 2                  # (more than one BGZF member)


# ------------------------------------------------------------------------------------------ 2. fetch
def windows_of(path, lengths, shapes, n=200, seed=20261018):
    """`n` windows (tid, beg, end): starts at 0, ends at the contig's end, windows across bin boundaries of every level of every
    shape next to a record, and random ones around records and anywhere"""
    rng = random.Random(seed)
    recs = [r for r in linear_records(path) if r[2] >= 0]
    out = []
    tids = sorted({r[2] for r in recs})
    for tid in tids[:3]:
        first = min(r[3] for r in recs if r[2] == tid)
        last = max(r[4] for r in recs if r[2] == tid)
        out += [(tid, 0, first + 150), (tid, 0, 1), (tid, last - 150, lengths[tid]), (tid, lengths[tid] - 1, lengths[tid]), (tid, 0, lengths[tid])]
    for min_shift, depth in shapes:
        for level in range(1, depth + 1):
            shift = min_shift + 3 * (depth - level)
            _name, _flag, tid, pos, end = rng.choice(recs)
            for edge in ((pos >> shift) << shift, ((end >> shift) + 1) << shift):
                if 0 < edge < lengths[tid]:
                    out.append((tid, max(0, edge - rng.randint(1, 400)), min(lengths[tid], edge + rng.randint(1, 400))))
    while len(out) < n:
        _name, _flag, tid, pos, end = rng.choice(recs)
        if rng.random() < 0.2:
            beg = rng.randrange(lengths[tid])
        else:
            beg = max(0, pos + rng.randint(-700, 200))
        out.append((tid, beg, min(lengths[tid], beg + rng.choice([1, 2, 50, 300, 700]))))
    return out[:n]


@pytest.mark.parametrize("label", LABELS)
def test_fetch_is_the_linear_scan(inputs, copies, label):
    """the Python reader on every CSI shape, the Python reader on the BAI copy and the overlap rule over the whole file"""
    _sites, sample, nbam, shapes = inputs[label]
    with_bai = sample.bam
    recs = [r for r in linear_records(nbam.filename) if r[2] >= 0]
    tid_a = np.array([r[2] for r in recs])
    pos_a = np.array([r[3] for r in recs], np.int64)
    end_a = np.array([r[4] for r in recs], np.int64)
    wins = windows_of(nbam.filename, with_bai.lengths, shapes)
    assert len(wins) == 200
    key = lambda it: [(r.query_name, r.flag, r.reference_start) for r in it]
    want, hits = [], 0
    for tid, beg, end in wins:
        picked = np.nonzero((tid_a == tid) & (pos_a < end) & (end_a > beg))[0]
        scan = [(recs[i][0], recs[i][1], recs[i][3]) for i in picked]
        assert key(with_bai.fetch(with_bai.references[tid], beg, end)) == scan, (tid, beg, end)
        want.append(scan)
        hits += len(scan) > 0
    assert hits > 100
    for shape in shapes:
        with_csi = bam.AlignmentFile(copies(label, shape))
        for (tid, beg, end), scan in zip(wins, want):
            assert key(with_csi.fetch(with_csi.references[tid], beg, end)) == scan, (shape, tid, beg, end)


# ------------------------------------------------------------------------------------------ 3. records
def host_routes(sites, sample, nbam):
    """offsets, records and skip flags of svt_bam_evidence in both count modes (1 and 3 threads) and of the two host walks"""
    out = []
    for mode, max_reads, threads in ((nr.COUNT_SSO, 1000, 1), (nr.COUNT_CLASSIC, None, 3)):
        a = W.unit_arrays(sites, sample, nbam, mode)
        out.append(nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, threads)[:3])
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    for walk in (nbam.evidence_walk_host, nbam.evidence_walk_open_host):
        got = walk(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
        assert not np.asarray(got[3]).any(), "a unit left the walk's envelope"
        out.append(got[:3])
    return out


@pytest.fixture(scope="module")
def bai_routes(inputs):
    made = {}

    def get(label):
        if label not in made:
            sites, sample, nbam, _ = inputs[label]
            made[label] = host_routes(sites, sample, nbam)
        return made[label]
    return get


@pytest.mark.parametrize("label,shape", CASES)
def test_records_equal_the_bai_copys(inputs, copies, bai_routes, label, shape):
    sites, sample, _nbam, _ = inputs[label]
    want = bai_routes(label)
    got = host_routes(sites, sample, nr.NativeBam(copies(label, shape)))
    for k, (w, g) in enumerate(zip(want, got)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(w, g)), "route %d" % k
    assert len(want[0][1]) > 50


def test_long_contig_records_are_the_references(long_groups):
    import test_geometry_edges as E
    import test_native_reads as N
    from oracle import c_oracle
    from svtyper_amd.results import result_from_record
    assert [g["shift"] for g, *_ in long_groups] == [2 ** 29 - 110_000, 3 * 2 ** 29 + 12_345, 2 ** 31 - 2 ** 20]
    for grp, sites, sample, nbam in long_groups:
        assert nbam.index_info() == sample.bam.index_info() == {"kind": "csi", "min_shift": 14, "depth": 6}
        assert len(sites) == 20 and nbam.lengths == (2 ** 31 - 1, 2 ** 31 - 1)
        off, want = E.golden_unit_records(grp)
        for k, got in enumerate(host_routes(sites, sample, nbam)):
            assert not got[2].any() and np.array_equal(got[0], off), "route %d" % k
            E.assert_records_equal(got[1], want, "route %d" % k)
        # the Python reader on the BAM, and from its records the reference's tallies and results (CPU oracle engine)
        py = N._python_records(sites, sample, nr.COUNT_SSO, 1000)
        assert np.array_equal(py[0], off)
        E.assert_records_equal(py[1], want, "python reader")
        rows = [[int(x) for x in row] for row in py[1].tolist()]
        mine = [dict(s, records=rows[int(off[k]):int(off[k + 1])]) for k, s in enumerate(grp["sites"])]
        res = c_oracle.genotype_batch(gio.batch_from_sites(mine, grp["libraries"]), flags=ev.FLAG_SSO_ASSOCIATION)
        for k, s in enumerate(mine):
            for j, t in enumerate(gio.TALLIES):
                assert float(res.tallies[k, j]).hex() == s["tallies_sso"][t], (s["breakpoint"]["id"], t)
            gio.assert_result_equal(result_from_record(res.rec[k]), gio.golden_result(s["result"]), 0.0, s["breakpoint"]["id"])
    first = long_groups[0][0]["sites"]
    assert min(s["breakpoint"]["A"]["pos"] for s in first) < 2 ** 29 < max(s["breakpoint"]["B"]["pos"] for s in first)
    assert all(r[3] < 2 ** 31 - 700_000 for g, *_ in long_groups for s in g["sites"] for r in s["reads"])


def test_the_long_contig_golden_is_no_larger_than_the_fake_one():
    size = lambda name: os.path.getsize(os.path.join(gio.GOLDEN, name))
    assert size(CC.LONG_GOLDEN) <= size("fake_sites.json.gz")


# ------------------------------------------------------------------------------------------ 4. libraries
def test_sample_from_bam_writes_the_same_library_file(copies):
    g = gio.load("library_from_bam.json.gz")
    texts = {}
    for name, path in (("bai", W.FIXTURE_BAM), ("csi", copies("fixture", (14, 6)))):
        for native in (None, nr.NativeBam(path)):
            sample = library.Sample.from_bam(bam.AlignmentFile(path), 1000000, 1e-3, native)
            out = io.StringIO()
            out.close = lambda: None
            library.write_sample_json([sample], out)
            texts[(name, native is not None)] = out.getvalue().replace(json.dumps(path), json.dumps("x.bam"))
    assert len(set(texts.values())) == 1 and len(texts) == 4
    info = json.loads(texts[("csi", True)])[g["sample"]]
    assert (info["mapped"], info["unmapped"]) == (g["mapped"], g["unmapped"]) and info["bam"] == "x.bam"
    assert len(info["libraryArray"]) == len(g["libraries"])
    for got, want in zip(info["libraryArray"], g["libraries"]):
        assert got["library_name"] == want["name"] and got["readgroups"] == want["readgroups"] and got["read_length"] == want["read_length"]
        assert float(got["mean"]).hex() == want["mean"] and float(got["sd"]).hex() == want["sd"]
        assert float(got["prevalence"]).hex() == want["prevalence"] and got["histogram"] == want["hist"]


@pytest.mark.parametrize("shape", [(14, 5), (16, 5), (14, 6)])
@pytest.mark.parametrize("which", ["synthetic", "short"])
def test_library_walk_on_csi_cuts(workdir, which, shape):
    """svt_bam_scan_libraries_walk_host cut at the CSI's record starts against the host scan, at the default and at the
    smallest round; (16, 5) has a quarter of the leaf bins of a BAI's linear index"""
    src = os.path.join(str(workdir), which + "_libscan.bam")
    if not os.path.exists(src):
        (lc.write_synthetic(src, 2) if which == "synthetic" else lc.write_short(src))
    groups, n_records = (lc.GROUPS, 3000) if which == "synthetic" else ([["r0"], ["r1"]], 120000)
    with_bai = nr.NativeBam(src)
    with_csi = nr.NativeBam(CC.csi_only_copy(src, workdir / ("%s_libscan_%d_%d" % ((which,) + shape)), shape))
    assert with_csi.index_info()["kind"] == "csi"
    for round_bytes in (0, lc.SMALL_ROUND):
        for num_samp in (0, 150, 1000000):
            st = lc.compare(with_csi, groups, num_samp, round_bytes, expect_reason=lc.WALK)
            assert st["records_walked"] == n_records or which == "short"
            assert lc.host_scan(with_csi, groups, num_samp) == lc.host_scan(with_bai, groups, num_samp)
    st_bai = lc.compare(with_bai, groups, 0, 0, expect_reason=lc.WALK)
    st_csi = lc.compare(with_csi, groups, 0, 0, expect_reason=lc.WALK)
    assert st_csi["segments"] > 1
    if shape == (16, 5) and which == "synthetic":
        assert st_csi["segments"] < st_bai["segments"]


# ------------------------------------------------------------------------------------------ 5. drivers
def oracle_engine(batch, flags=0):
    from oracle import c_oracle
    return c_oracle.genotype_batch(batch, flags=flags)


@pytest.mark.parametrize("reader", ["native", "python"])
@pytest.mark.parametrize("driver", ["sso", "classic"])
def test_drivers_on_the_csi_only_fixture(tmp_path, copies, driver, reader):
    import test_host_pipeline as T
    out = str(tmp_path / "out.vcf")
    path = copies("fixture", (14, 6))
    with open(EXAMPLE_VCF) as inf, open(out, "w") as outf:
        if driver == "sso":
            singlesample.sso_genotype(path, inf, outf, 20, 1, 1, 1000000, LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                      engine=oracle_engine, reader=reader)
        else:
            classic.sv_genotype(path, inf, outf, 20, 1, 1, 1000000, LIB_JSON, False, None, None, False, None, 1e10,
                                engine=oracle_engine, reader=reader)
    T.same_vcf(EXPECTED_VCF, out)


@pytest.mark.parametrize("reader", ["native", "python"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_three_bams_with_one_of_them_csi_only(tmp_path, which, reader):
    import test_multisample_qual as M
    bams, vcf_path, lib_json = M.three_sample_case(str(tmp_path))
    paths = bams.split(",")
    os.remove(paths[which] + ".bai")
    csiwriter.write_csi(paths[which], paths[which] + ".csi", *((14, 6), (10, 3), (16, 5))[which])
    assert [nr.NativeBam(p).index_info()["kind"] for p in paths] == ["csi" if k == which else "bai" for k in range(3)]
    out = str(tmp_path / "three_out.vcf")
    with open(vcf_path) as inf, open(out, "w") as outf:
        classic.sv_genotype(bams, inf, outf, 20, 1, 1, 1000000, lib_json, False, None, None, False, None, 1e10,
                            engine=oracle_engine, reader=reader)
    M._same([l for l in open(out).read().split("\n") if not l.startswith("##fileDate=")], M._golden(False))


# ------------------------------------------------------------------------------------------ 6. precedence and errors
def small_bam(directory, name="p.bam"):
    os.makedirs(str(directory), exist_ok=True)
    path = os.path.join(str(directory), name)
    bw.write_bam(path, W.HEADER, [("1", 100000), ("2", 100000)], [W._read("r%03d" % k, 40_000 + 37 * k) for k in range(300)], block_bytes=900)
    return path


def both_refuse(path, match):
    with pytest.raises(hip.SvtyperHipError, match=match):
        nr.NativeBam(path)
    with pytest.raises(IOError, match=match):
        bam.AlignmentFile(path)


def test_bai_comes_first_and_the_magic_decides(tmp_path):
    path = small_bam(tmp_path / "both")
    csiwriter.write_csi(path, path + ".csi", 14, 6)
    assert nr.NativeBam(path).index_info()["kind"] == "bai" and bam.AlignmentFile(path).index_info()["kind"] == "bai"
    # ... the .bai next to the file (the stem's) still comes before <path>.csi
    os.replace(path + ".bai", path[:-4] + ".bai")
    assert nr.NativeBam(path).index_info()["kind"] == "bai" and bam.AlignmentFile(path).index_info()["kind"] == "bai"
    os.remove(path[:-4] + ".bai")
    assert nr.NativeBam(path).index_info() == {"kind": "csi", "min_shift": 14, "depth": 6}
    os.replace(path + ".csi", path[:-4] + ".csi")
    assert nr.NativeBam(path).index_info()["kind"] == "csi" and bam.AlignmentFile(path).index_info()["kind"] == "csi"
    # a BAI under the name of a CSI and a CSI under the name of a BAI are what their magic says
    swapped = small_bam(tmp_path / "swapped")
    os.replace(swapped + ".bai", swapped + ".csi")
    assert nr.NativeBam(swapped).index_info()["kind"] == "bai" and bam.AlignmentFile(swapped).index_info()["kind"] == "bai"
    csiwriter.write_csi(swapped, swapped + ".bai", 13, 6)
    want = {"kind": "csi", "min_shift": 13, "depth": 6}
    assert nr.NativeBam(swapped).index_info() == want and bam.AlignmentFile(swapped).index_info() == want
    want_names = [r.query_name for r in bam.AlignmentFile(path).fetch("1", 41_000, 42_000)]
    assert [r.query_name for r in bam.AlignmentFile(swapped).fetch("1", 41_000, 42_000)] == want_names and len(want_names) > 20


def test_without_an_index_the_text_is_the_old_one_and_more(tmp_path):
    path = small_bam(tmp_path / "none")
    os.remove(path + ".bai")
    with pytest.raises(hip.SvtyperHipError, match=r"no \.bai index found for .*p\.bam \(nor a \.csi\)"):
        nr.NativeBam(path)
    plain = bam.AlignmentFile(path)                    # (the Python reader opens, as before, and cannot fetch)
    assert plain.index_info() is None
    with pytest.raises(ValueError, match="without index"):
        list(plain.fetch("1", 0, 10))


def csi_error_cases(directory):
    """name -> path of a BAM whose only index is a broken CSI, and what the error has to say besides the index's name"""
    path = small_bam(directory / "src")
    whole = csiwriter.csi_bytes(path, 14, 6)
    packed = csiwriter.bgzf(whole, 700)
    header = lambda min_shift, depth: whole[:4] + struct.pack("<ii", min_shift, depth) + whole[12:]
    flipped = bytearray(packed)
    flipped[18 + 40] ^= 0x5A                                           # inside the first member's deflate stream
    n_ref_at = 16
    bin_at = n_ref_at + 4                                              # n_bin of the first reference
    cases = {
        "cut_in_a_member": (packed[:len(packed) // 2], "truncated|inflate|BGZF"),
        "cut_between_members": (csiwriter.bgzf(whole[:len(whole) // 2], 700), "truncated"),
        "cut_in_the_header": (csiwriter.bgzf(whole[:10]), "truncated"),
        "flipped_byte": (bytes(flipped), "inflate|CRC32"),
        "wrong_magic": (csiwriter.bgzf(b"CSJ\1" + whole[4:]), "not a CSI index"),
        "tabix_magic": (csiwriter.bgzf(b"TBI\1" + whole[4:]), "not a CSI index"),
        "negative_min_shift": (csiwriter.bgzf(header(-1, 6)), "min_shift"),
        "negative_depth": (csiwriter.bgzf(header(14, -2)), "depth"),
        "shift_beyond_62": (csiwriter.bgzf(header(39, 8)), "min_shift"),
        "negative_l_aux": (csiwriter.bgzf(whole[:12] + struct.pack("<i", -5) + whole[16:]), "negative"),
        "negative_n_ref": (csiwriter.bgzf(whole[:n_ref_at] + struct.pack("<i", -1) + whole[n_ref_at + 4:]), "negative"),
        "negative_n_bin": (csiwriter.bgzf(whole[:bin_at] + struct.pack("<i", -3) + whole[bin_at + 4:]), "negative"),
        "negative_n_chunk": (csiwriter.bgzf(whole[:bin_at + 16] + struct.pack("<i", -1) + whole[bin_at + 20:]), "negative"),
        "huge_n_chunk": (csiwriter.bgzf(whole[:bin_at + 16] + struct.pack("<i", 2 ** 30) + whole[bin_at + 20:]), "truncated"),
        "huge_n_ref": (csiwriter.bgzf(whole[:n_ref_at] + struct.pack("<i", 2 ** 31 - 1) + whole[n_ref_at + 4:]), "truncated"),
    }
    out = {}
    for name, (data, match) in cases.items():
        d = os.path.join(str(directory), name)
        os.makedirs(d)
        dst = os.path.join(d, "p.bam")
        shutil.copy(path, dst)
        with open(dst + ".csi", "wb") as f:
            f.write(data)
        out[name] = (dst, match)
    os.makedirs(os.path.join(str(directory), "clean"))
    clean = os.path.join(str(directory), "clean", "p.bam")
    shutil.copy(path, clean)
    with open(clean + ".csi", "wb") as f:
        f.write(packed)
    return out, clean


@pytest.fixture(scope="module")
def broken(workdir):
    return csi_error_cases(workdir / "broken")


@pytest.mark.parametrize("name", ["cut_in_a_member", "cut_between_members", "cut_in_the_header", "flipped_byte", "wrong_magic", "tabix_magic",
                                  "negative_min_shift", "negative_depth", "shift_beyond_62", "negative_l_aux", "negative_n_ref",
                                  "negative_n_bin", "negative_n_chunk", "huge_n_chunk", "huge_n_ref"])
def test_a_broken_csi_is_refused_with_its_name(broken, name):
    cases, clean = broken
    assert nr.NativeBam(clean).index_info() == bam.AlignmentFile(clean).index_info() == {"kind": "csi", "min_shift": 14, "depth": 6}
    path, match = cases[name]
    both_refuse(path, r"p\.bam\.csi.*(%s)" % match)


def test_a_truncated_bai_under_either_name_is_refused_with_its_name(tmp_path):
    path = small_bam(tmp_path / "cutbai")
    data = open(path + ".bai", "rb").read()
    with open(path + ".bai", "wb") as f:
        f.write(data[:len(data) // 2])
    with pytest.raises(hip.SvtyperHipError, match=r"truncated BAI.*p\.bam\.bai"):
        nr.NativeBam(path)
    os.replace(path + ".bai", path + ".csi")
    with pytest.raises(hip.SvtyperHipError, match=r"truncated BAI.*p\.bam\.csi"):
        nr.NativeBam(path)
    with open(path + ".csi", "wb") as f:
        f.write(data[:3])                                                       # not even a magic
    with pytest.raises(hip.SvtyperHipError, match=r"p\.bam\.csi is not a BAI index"):
        nr.NativeBam(path)
    with pytest.raises(IOError, match=r"p\.bam\.csi is not a BAI index"):
        bam.AlignmentFile(path)


# ------------------------------------------------------------------------------------------ 7. sanitizers
def test_index_header_under_asan_and_ubsan(tmp_path, broken):
    """svt_bam_index.h alone, in a stand-alone program: every broken CSI above and the clean one, then 1 000 random reg2bins /
    min_offset / fetch_chunks queries on the clean one"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cases, clean = broken
    exe = str(tmp_path / "asan_csi")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "asan_csi_main.cpp"), "-o", exe]
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("libasan" in r.stderr.lower() or "libubsan" in r.stderr.lower()):
        pytest.skip("this g++ has no AddressSanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    bad = [p + ".csi" for p, _ in cases.values()]
    r = subprocess.run([exe, clean + ".csi"] + bad, env=dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and not any(l.startswith("FAILED") for l in lines), lines
    assert lines[-2] == "1 loaded, %d refused, 1000 queries" % len(bad), lines[-2]

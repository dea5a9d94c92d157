"""`svtyper -w` over several ranks (sharded.sv_genotype_sharded(..., alignment_gather=True)): every rank's dump in a
bam.RecordSink, the sinks gathered onto rank 0, the first occurrence of every (query_name, flag) written once by rank 0 -- the
file of the one-process run.  CPU: gloo, torch.multiprocessing.spawn, world 2 and 3, the engine seam filled by
verdictcases.VerdictOracleEngine, reader="python"; the worker pattern of tests/test_sharded_drivers.py.  One spawn per world runs
all of that world's cases in one process group.  (tests/test_sharded_write_alignment_device.py: the CLI under
torch.distributed.run on the GPU.)"""
import io
import json
import os
import subprocess
import sys
import time

import pytest

import test_host_pipeline as T
import test_sharded_drivers as S
import test_write_alignment_host as W
import test_write_alignment_walk_host as H
import verdictcases as V
from svtyper_amd import classic, sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAWN_TIMEOUT = 300

# name -> keywords of the run; "gather": handed to the sharded driver only
CASES = {
    "plain": dict(),
    "bai": dict(alignment_sort=True, alignment_index="bai", deflate="host"),
    "csi": dict(alignment_sort=True, alignment_index="csi", deflate="host"),
    "dynamic": dict(alignment_sort=True, deflate="host", huffman="dynamic"),
}
# (g) what every rank must refuse alike, in front of the first collective
REFUSED = {
    "index": (dict(alignment_index="tbi"), "alignment_index must be"),
    "huffman": (dict(huffman="dynamic"), "huffman='dynamic' needs"),
    "deflate": (dict(deflate="gpu"), "deflate must be"),
    "reader": (dict(reader="native"), "keeps no reads"),
    "geometry": (dict(geometry="device"), "no canonical records"),
    "engine": (dict(engine=T.oracle_engine), "supports_verdicts"),
}


def make_input(tmp_path, first=8, last=8):
    """A slice of the fixture's body that holds its BND pair -- `first` lines from the first mate on, the `last` lines up to the
    second mate --, then a copy of the slice's other lines with _b behind the ID: the later ranks meet reads of the earlier ones."""
    lines = open(T.IN_VCF).read().splitlines(True)
    head = [l for l in lines if l.startswith("#")]
    body = [l for l in lines if not l.startswith("#")]
    bnd = [i for i, l in enumerate(body) if "SVTYPE=BND" in l]
    assert len(bnd) == 2
    chosen = body[bnd[0]:bnd[0] + first] + body[bnd[1] + 1 - last:bnd[1] + 1]
    again = []
    for l in chosen:
        if "SVTYPE=BND" not in l:
            cols = l.split("\t")
            cols[2] += "_b"
            again.append("\t".join(cols))
    path = str(tmp_path / "in.vcf")
    with open(path, "w") as f:
        f.write("".join(head + chosen + again))
    return path, len(chosen) + len(again)


def make_tiny_input(tmp_path):
    """two lines, the second a copy of the first: with three ranks the last one has no line, and rank 1 meets rank 0's reads only"""
    lines = open(T.IN_VCF).read().splitlines(True)
    head = [l for l in lines if l.startswith("#")]
    line = [l for l in lines if not l.startswith("#") and "SVTYPE=BND" not in l][3]
    cols = line.split("\t")
    cols[2] += "_b"
    path = str(tmp_path / "tiny_in.vcf")       # (not where rank 0 writes the job's output)
    with open(path, "w") as f:
        f.write("".join(head + [line, "\t".join(cols)]))
    return path


def _args(out_bam):
    return (20, 1, 1, 1000000, T.LIB_JSON, False, out_bam, None, False, None, 1e10)


def single(in_path, out_bam, **kw):
    """the one-process run: its VCF text"""
    sink = sharded._Sink()
    with open(in_path) as f:
        classic.sv_genotype(T.IN_BAM, f, sink, *_args(out_bam), engine=V.VerdictOracleEngine(), **kw)
    return sink.getvalue()


def _worker(rank, world, port, jobs, out_dir):
    """jobs: [(name, in_path or None, keywords, gather)]; rank r notes what became of each in out_dir/<name>.rank<r>"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for name, in_path, kw, gather in jobs:
        kw = dict(kw)
        kw.setdefault("engine", V.VerdictOracleEngine())
        out_bam = os.path.join(out_dir, name + ".bam")
        out = open(os.path.join(out_dir, name + ".vcf"), "w") if rank == 0 else io.StringIO()
        stats = {}
        note = {}
        try:
            f = open(in_path) if in_path is not None else None
            sharded.sv_genotype_sharded(T.IN_BAM, f, out, *_args(out_bam), rank=rank, world=world, stats=stats, **kw,
                                        **({"alignment_gather": True} if gather else {}))
            note["verdict"] = "ran"
            note["gather"] = stats.get("alignment_gather")
            if rank != 0:
                assert out.getvalue() == ""
        except ValueError as e:
            note["verdict"] = "ValueError: %s" % e
        if rank == 0:
            out.close()
        with open(os.path.join(out_dir, "%s.rank%d" % (name, rank)), "w") as g:
            json.dump(note, g)
    sharded.finish()


def spawn(world, jobs, out_dir):
    """the spawn joins within its timeout, or the test fails with the workers gone"""
    import torch.multiprocessing as mp
    ctx = mp.spawn(_worker, args=(world, S._free_port(), jobs, out_dir), nprocs=world, join=False)
    deadline = time.time() + SPAWN_TIMEOUT
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish within %d s: one of them waits in a collective" % SPAWN_TIMEOUT)


def notes(out_dir, name, world):
    return [json.load(open(os.path.join(out_dir, "%s.rank%d" % (name, r)))) for r in range(world)]


@pytest.fixture(scope="module")
def one_process(tmp_path_factory):
    """the input, and per case the one-process run's files"""
    tmp = tmp_path_factory.mktemp("one_process")
    in_path, n_lines = make_input(tmp)
    runs = {}
    for name, kw in CASES.items():
        out_bam = str(tmp / (name + ".bam"))
        runs[name] = (out_bam, single(in_path, out_bam, **kw))
    return in_path, n_lines, runs


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory, one_process):
    in_path, _n, _runs = one_process
    out_dir = str(tmp_path_factory.mktemp("two_ranks"))
    jobs = [(name, in_path, kw, True) for name, kw in CASES.items()]
    jobs += [("refused_" + name, in_path, kw, True) for name, (kw, _text) in REFUSED.items()]
    jobs += [("no_gather", in_path, {}, False), ("header_only", None, {}, True)]
    spawn(2, jobs, out_dir)
    return out_dir


@pytest.fixture(scope="module")
def three_ranks(tmp_path_factory, one_process):
    in_path, _n, _runs = one_process
    tmp = tmp_path_factory.mktemp("three_ranks")
    tiny = make_tiny_input(tmp)
    tiny_bam = str(tmp / "tiny_single.bam")
    tiny_vcf = single(tiny, tiny_bam, **CASES["bai"])
    spawn(3, [("plain", in_path, CASES["plain"], True), ("tiny", tiny, CASES["bai"], True)], str(tmp))
    return str(tmp), tiny_bam, tiny_vcf


def test_the_premise(one_process, two_ranks, three_ranks):
    """the dump is not a toy, the ranks really meet each other's reads, and the cross-rank pass really drops some"""
    in_path, n_lines, runs = one_process
    n_single = len(V.written_records(runs["plain"][0])[0])
    assert n_single >= 1000
    body = [l for l in open(in_path) if not l.startswith("#")]
    assert len(body) == n_lines and all(sharded.plan_shards(body, w)[r] for w in (2, 3) for r in range(w))
    for out_dir, world in ((two_ranks, 2), (three_ranks[0], 3)):
        g = notes(out_dir, "plain", world)[0]["gather"]
        print(world, g)
        assert len(g["records_per_rank"]) == world and all(c > 0 for c in g["records_per_rank"])
        assert g["records"] == sum(g["records_per_rank"]) and g["kept"] == n_single
        assert g["records"] - g["kept"] >= 1            # dropped by the pass over the ranks, not by a rank's own set
        assert all(n["gather"] is None for n in notes(out_dir, "plain", world)[1:])


@pytest.mark.parametrize("world", [2, 3])
def test_unsorted_payload_and_vcf_are_the_one_process_runs(one_process, two_ranks, three_ranks, world):
    """(a), (d)"""
    _in, _n, runs = one_process
    out_dir = two_ranks if world == 2 else three_ranks[0]
    want_bam, want_vcf = runs["plain"]
    assert all(n["verdict"] == "ran" for n in notes(out_dir, "plain", world))
    assert H.payload(os.path.join(out_dir, "plain.bam")) == H.payload(want_bam)
    assert V.written_records(os.path.join(out_dir, "plain.bam")) == V.written_records(want_bam)       # (every member's CRC32 checked)
    assert W.no_date(open(os.path.join(out_dir, "plain.vcf")).read()) == W.no_date(want_vcf)


@pytest.mark.parametrize("case, index", [("bai", ".bai"), ("csi", ".csi"), ("dynamic", None)])
def test_sorted_and_indexed_files_are_byte_identical(one_process, two_ranks, case, index):
    """(b), (c), (d): deflate="host" makes the members a function of the records alone"""
    _in, _n, runs = one_process
    want_bam, want_vcf = runs[case]
    got_bam = os.path.join(two_ranks, case + ".bam")
    assert all(n["verdict"] == "ran" for n in notes(two_ranks, case, 2))
    assert open(got_bam, "rb").read() == open(want_bam, "rb").read()
    for ext in (".bai", ".csi"):
        assert os.path.exists(got_bam + ext) == os.path.exists(want_bam + ext) == (ext == index)
    if index:
        assert open(got_bam + index, "rb").read() == open(want_bam + index, "rb").read()
    assert W.no_date(open(os.path.join(two_ranks, case + ".vcf")).read()) == W.no_date(want_vcf)
    assert len(V.written_records(got_bam)[0]) >= 1000


def test_a_rank_without_lines(three_ranks):
    """(e) world 3 over two lines: rank 2 has nothing, rank 1 nothing new -- the file is rank 0's, sorted and indexed"""
    out_dir, want_bam, want_vcf = three_ranks
    ns = notes(out_dir, "tiny", 3)
    assert all(n["verdict"] == "ran" for n in ns)
    g = ns[0]["gather"]
    assert g["records_per_rank"][2] == 0 and g["records_per_rank"][0] == g["records_per_rank"][1] == g["kept"] > 0
    got_bam = os.path.join(out_dir, "tiny.bam")
    assert open(got_bam, "rb").read() == open(want_bam, "rb").read()
    assert open(got_bam + ".bai", "rb").read() == open(want_bam + ".bai", "rb").read()
    assert W.no_date(open(os.path.join(out_dir, "tiny.vcf")).read()) == W.no_date(want_vcf)


def test_without_the_option_the_call_is_refused_as_before(two_ranks):
    """(f)"""
    for n in notes(two_ranks, "no_gather", 2):
        assert n["verdict"].startswith("ValueError") and "every rank would write the same file" in n["verdict"]
        assert "--gather-alignment" in n["verdict"]
    assert not os.path.exists(os.path.join(two_ranks, "no_gather.bam"))


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_an_option_error_is_every_ranks(two_ranks, name):
    """(g) every rank raises alike and in front of the first collective: the spawn of the fixture joined, the jobs behind ran"""
    for n in notes(two_ranks, "refused_" + name, 2):
        assert n["verdict"].startswith("ValueError") and REFUSED[name][1] in n["verdict"], n
    assert not os.path.exists(os.path.join(two_ranks, "refused_%s.bam" % name))
    assert all(n["verdict"] == "ran" for n in notes(two_ranks, "header_only", 2))


def test_without_a_vcf_rank_zero_writes_the_header_only_bam(two_ranks):
    f, records = W.all_records(os.path.join(two_ranks, "header_only.bam"))
    f.close()
    assert records == []
    assert open(os.path.join(two_ranks, "header_only.bam"), "rb").read()[-28:] == W.bam.BGZF_EOF


def test_usage_errors_in_one_process(tmp_path):
    with open(T.IN_VCF) as f, pytest.raises(ValueError, match="needs -w"):
        sharded.sv_genotype_sharded(T.IN_BAM, f, io.StringIO(), *_args(None), rank=0, world=2, alignment_gather=True,
                                    engine=V.VerdictOracleEngine())
    with open(T.IN_VCF) as f, pytest.raises(ValueError, match="several ranks"):
        sharded.sv_genotype_sharded(T.IN_BAM, f, io.StringIO(), *_args(str(tmp_path / "x.bam")), rank=0, world=1, alignment_gather=True,
                                    engine=V.VerdictOracleEngine())
    assert not os.path.exists(str(tmp_path / "x.bam"))


def test_cli_usage_errors(tmp_path):
    """--gather-alignment in one process, and without -w: usage errors (status 2), nothing written"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    base = [sys.executable, "-m", "svtyper_amd.classic", "-i", T.IN_VCF, "-B", T.IN_BAM, "-l", T.LIB_JSON, "-o", str(tmp_path / "o.vcf")]
    r = subprocess.run(base + ["-w", str(tmp_path / "o.bam"), "--gather-alignment"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "several ranks" in r.stderr and not os.path.exists(str(tmp_path / "o.bam"))
    r = subprocess.run(base + ["--gather-alignment"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs -w" in r.stderr

"""GPU: the line table, the gather and the one-call entry of the sorted, tabix-indexed BGZF output on the device
(svt_vcf_lines_kernel.h) against their host twins and the checker of tests/tbxcases.py; the writer with deflate="device" against
the files deflate="host" writes, byte for byte; sso_genotype over the fixture, sorted and indexed; the command line in a child
process."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import tbxcases as X
import test_host_pipeline as T
from svtyper_amd import bam, bgzf_out, singlesample
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def as_tuples(lines):
    return [tuple(int(v) for v in row) for row in lines.tolist()]


def write(path, text, **options):
    out = bgzf_out.open_text(path, **options)
    out.write(text.decode())
    out.close()
    return open(path, "rb").read()


@pytest.mark.parametrize("shift", [0, 1, 15])
def test_device_line_table_is_the_hosts_and_the_checkers(hip_device, shift):
    """every text of the corpus, moved against the tiles by `shift` header bytes"""
    for name in sorted(X.TABLE_TEXTS):
        text = (b"#" * (shift - 1) + b"\n" if shift else b"") + X.TABLE_TEXTS[name]
        got = nr.vcf_lines(text, device=hip_device)
        assert as_tuples(got) == X.table(text), name
        assert got.tobytes() == nr.vcf_lines(text).tobytes(), name


def test_device_gather_is_the_hosts(hip_device):
    rng = np.random.default_rng(5)
    for name in sorted(X.TEXTS) + sorted(X.ORDERS):
        text = X.TEXTS.get(name, X.ORDERS.get(name))
        lines = nr.vcf_lines(text)
        orders = [np.arange(len(lines))[::-1], rng.permutation(len(lines)), np.arange(len(lines))[: len(lines) // 2]]
        if not text or text.endswith(b"\n"):
            perm, bad = nr.vcf_sort_order(text, lines)
            assert bad == 0
            orders.append(perm)
        for perm in orders:
            assert nr.vcf_gather(text, lines, perm, device=hip_device) == nr.vcf_gather(text, lines, perm), name


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
@pytest.mark.parametrize("sort", [False, True])
def test_one_call_entry(hip_device, huffman, sort):
    for name in sorted(X.TEXTS) + sorted(X.ORDERS):
        text = X.TEXTS.get(name, X.ORDERS.get(name))
        if sort and text and not text.endswith(b"\n"):
            text += b"\n"
        members, out_off, lines, src_off, bad = nr.vcf_bgzf_device(text, sort, huffman, hip_device)
        assert bad == 0
        written = X.sorted_text(text) if sort else text
        payloads = [written[at:at + X.PAYLOAD] for at in range(0, len(written), X.PAYLOAD)]
        want, want_off = nr.bgzf_deflate(payloads, device=hip_device, huffman=huffman)
        assert members.tobytes() == want.tobytes() and out_off.tolist() == want_off.tolist(), name
        assert gzip.decompress(members.tobytes()) == written if written else len(members) == 0
        assert lines.tobytes() == nr.vcf_lines(written).tobytes(), name
        assert all(text[int(s):int(s) + int(l["len"])] == written[int(l["off"]):int(l["off"]) + int(l["len"])] for s, l in zip(src_off, lines)), name
    text = X.HEADER + X.vcf_line(1, 5, "a") + X.LINES["seven_columns"][0]
    assert nr.vcf_bgzf_device(text, True, huffman, hip_device)[4] == 4
    times = nr.vcf_lines_last_times()
    assert set(times) == {"count_kernel_s", "starts_kernel_s", "parse_kernel_s", "gather_kernel_s", "total_s"} and times["count_kernel_s"] > 0


def test_times_of_sorted_and_unsorted_calls(hip_device):
    """every kernel of a call is timed between marks of its own (the gather's are not the parse's), and nothing of one call is
    left in the next one's times on the same thread"""
    text = X.ORDERS["contig_reappears"]
    if not text.endswith(b"\n"):
        text += b"\n"
    assert X.sorted_text(text) != text              # (its lines really move)
    kernels = ("count_kernel_s", "starts_kernel_s", "parse_kernel_s", "gather_kernel_s")
    assert nr.vcf_bgzf_device(text, True, "fixed", hip_device)[4] == 0
    times, deflate = nr.vcf_lines_last_times(), nr.bgzf_deflate_last_times()
    print("sorted", times, deflate)
    assert all(times[k] > 0 for k in kernels)
    assert deflate["crc_kernel_s"] > 0 and deflate["deflate_kernel_s"] > 0 and deflate["pack_kernel_s"] > 0
    assert times["total_s"] >= sum(times[k] for k in kernels) + deflate["crc_kernel_s"] + deflate["deflate_kernel_s"] + deflate["pack_kernel_s"]
    assert nr.vcf_bgzf_device(text, False, "fixed", hip_device)[4] == 0
    times = nr.vcf_lines_last_times()
    print("unsorted", times)
    assert times["gather_kernel_s"] == 0.0 and all(times[k] > 0 for k in kernels[:3])


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_writer_on_the_device_writes_the_hosts_files(tmp_path, hip_device, huffman):
    for k, name in enumerate(sorted(X.TEXTS) + sorted(X.ORDERS)):
        text = X.TEXTS.get(name, X.ORDERS.get(name))
        raw = {}
        for deflate in ("host", "device"):
            path = str(tmp_path / ("%s%d.vcf.gz" % (deflate, k)))
            raw[deflate] = (write(path, text, deflate=deflate, huffman=huffman, device=hip_device, sort=True, index="tbi"),
                            open(path + ".tbi", "rb").read())
        assert raw["device"] == raw["host"], name
        assert gzip.decompress(raw["device"][0]) == X.sorted_text(text)
        X.check_structure(raw["device"][0], X.read_tbi(raw["device"][1]))


def test_writer_on_the_device_without_sort(tmp_path, hip_device):
    text = X.ORDERS["contig_reappears"]
    path = str(tmp_path / "u.vcf.gz")
    out = bgzf_out.open_text(path, deflate="device", device=hip_device, index="tbi")
    out.write(text.decode())
    with pytest.raises(bgzf_out.VcfOrderError, match="--sort") as err:
        out.close()
    assert err.value.line == X.first_out_of_order(text) and not os.path.exists(path + ".tbi")
    assert open(path, "rb").read() == write(str(tmp_path / "p.vcf.gz"), text, deflate="host")
    text = X.TEXTS["spans_three_members"]
    raw = write(str(tmp_path / "i.vcf.gz"), text, deflate="device", device=hip_device, index="tbi")
    assert raw == write(str(tmp_path / "h.vcf.gz"), text, deflate="host", index="tbi")
    assert open(str(tmp_path / "i.vcf.gz.tbi"), "rb").read() == open(str(tmp_path / "h.vcf.gz.tbi"), "rb").read()
    tbi = X.read_tbi(open(str(tmp_path / "i.vcf.gz.tbi"), "rb").read())
    X.check_queries(raw, tbi, X.regions_of(text))


def no_date(data):
    return [l for l in data.split(b"\n") if not l.startswith(b"##fileDate=")]


def contig_blocks(text):
    blocks = []
    for line in X.split_lines(text):
        if not line.startswith(b"#"):
            chrom = line.split(b"\t")[0]
            if blocks and blocks[-1][0] == chrom:
                blocks[-1][1] += 1
            else:
                blocks.append([chrom, 1])
    return [tuple(b) for b in blocks]


def run_sso(out):
    with open(T.IN_VCF) as inf:
        singlesample.sso_genotype(T.IN_BAM, inf, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000)


def test_sso_fixture_sorted_and_indexed(tmp_path, hip_device):
    path = str(tmp_path / "sorted.vcf.gz")
    out = bgzf_out.open_text(path, deflate="device", device=hip_device, sort=True, index="tbi")
    run_sso(out)
    out.close()
    raw = open(path, "rb").read()
    text = gzip.decompress(raw)
    expected = open(T.EXPECTED, "rb").read()
    assert no_date(text) == no_date(X.sorted_text(expected)) and sorted(no_date(text)) == sorted(no_date(expected))
    assert contig_blocks(text) == [(b"2", 114), (b"3", 97), (b"15", 1)]
    tbi = X.read_tbi(open(path + ".tbi", "rb").read())
    members = X.Members(raw)
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(text), members)


def test_sso_fixture_without_sort_names_the_second_block(tmp_path, hip_device):
    path = str(tmp_path / "unsorted.vcf.gz")
    out = bgzf_out.open_text(path, deflate="device", device=hip_device, index="tbi")
    run_sso(out)
    with pytest.raises(bgzf_out.VcfOrderError) as err:
        out.close()
    text = gzip.decompress(open(path, "rb").read())
    number = X.first_out_of_order(text)                 # (from the checker, not from the product)
    lines = X.split_lines(text)
    assert err.value.line == number and "line %d (2:" % number in str(err.value)
    assert lines[number - 1].startswith(b"2\t") and lines[number - 2].startswith(b"3\t")
    assert no_date(text) == no_date(open(T.EXPECTED, "rb").read()) and not os.path.exists(path + ".tbi")


def test_command_line_sort_and_tabix_on_the_device(tmp_path, hip_device):
    """`--bgzf --sort --tabix -o PATH --deflate device`, then the file it wrote as `-i` of a second run; and the exit without --sort"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, "-m", "svtyper_amd.singlesample", "-B", T.IN_BAM, "-l", T.LIB_JSON]
    path = str(tmp_path / "cli.vcf.gz")
    r = subprocess.run(common + ["-i", T.IN_VCF, "--bgzf", "--sort", "--tabix", "-o", path, "--deflate", "device"], env=env, cwd=ROOT,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = open(path, "rb").read()
    text = gzip.decompress(raw)
    assert no_date(text) == no_date(X.sorted_text(open(T.EXPECTED, "rb").read())) and raw.endswith(bam.BGZF_EOF)
    tbi = X.read_tbi(open(path + ".tbi", "rb").read())
    X.check_structure(raw, tbi)
    assert X.query(raw, tbi, b"15", 0, X.TBI_END) == [l for l in X.split_lines(text) if l.startswith(b"15\t")]
    # a .vcf.gz as -i: the same output bytes as the plain file
    packed_in = str(tmp_path / "in.vcf.gz")
    write(packed_in, open(T.IN_VCF, "rb").read(), deflate="device", device=hip_device)
    outs = []
    for vcf_in in (T.IN_VCF, packed_in):
        r = subprocess.run(common + ["-i", vcf_in], env=env, cwd=ROOT, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(no_date(r.stdout))
    assert outs[0] == outs[1] and len(outs[0]) > 200
    r = subprocess.run(common + ["-i", T.IN_VCF, "--bgzf", "--tabix", "-o", str(tmp_path / "u.vcf.gz"), "--deflate", "device"], env=env, cwd=ROOT,
                       capture_output=True, timeout=600)
    unsorted = gzip.decompress(open(str(tmp_path / "u.vcf.gz"), "rb").read())
    assert r.returncode != 0 and b"--sort" in r.stderr and b"line %d (2:" % X.first_out_of_order(unsorted) in r.stderr
    assert not os.path.exists(str(tmp_path / "u.vcf.gz.tbi"))

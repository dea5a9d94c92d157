"""GPU: the span table, the radix sort and the one-call entry of the coordinate-sorted, BAI-indexed `-w` BAM on the device
(svt_bam_sort_kernel.h, svt_radix_sort_kernel.h) against their host twins and the checker of tests/baicases.py; the writer with deflate="device" against
the files deflate="host" writes, byte for byte; sv_genotype -w over the fixture, sorted and indexed, in process with the Python
reader and as the command line in a child process with the device reader."""
import os
import subprocess
import sys

import numpy as np
import pytest

import baicases as B
import test_bam_sort_host as H
import test_host_pipeline as T
from svtyper_amd import bam, classic
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_of(case, with_header=True):
    head = case.header if with_header else b""
    rec_off = np.cumsum([len(head)] + [len(r) for r in case.records]).astype(np.uint64)
    return head + b"".join(case.records), rec_off


def test_device_spans_and_order_are_the_hosts_and_the_checkers(hip_device):
    for name in sorted(B.CASES):
        case = B.CASES[name]
        data, rec_off = stream_of(case)
        spans, key_and, key_or = nr.bam_spans(data, rec_off, case.n_ref, device=hip_device)
        host, host_and, host_or = nr.bam_spans(data, rec_off, case.n_ref)
        assert spans.tobytes() == host.tobytes() and (key_and, key_or) == (host_and, host_or), name
        assert H.span_rows(spans) == B.table(len(case.header), case.records, case.n_ref), name
        perm, bad, kind = nr.bam_sort_order(spans, device=hip_device)
        assert (bad, kind) == B.first_bad(case.records, case.n_ref), name
        if not bad:
            assert perm.tobytes() == nr.bam_sort_order(host)[0].tobytes() and perm.tolist() == B.order(case.records, case.n_ref), name


@pytest.mark.parametrize("which, passes", [("single_pass", 1), ("every_digit", 8)])
def test_both_kinds_of_sorting_pass_run(hip_device, which, passes):
    case = B.single_pass_case() if which == "single_pass" else B.every_digit_case()
    data, rec_off = stream_of(case, with_header=False)
    spans, key_and, key_or = nr.bam_spans(data, rec_off, case.n_ref, device=hip_device)
    assert spans.tobytes() == nr.bam_spans(data, rec_off, case.n_ref)[0].tobytes()
    assert sum(1 for d in range(8) if (key_and ^ key_or) >> (8 * d) & 255) == passes
    perm, bad, _kind = nr.bam_sort_order(spans, device=hip_device)
    assert bad == 0 and perm.tolist() == B.order(case.records, case.n_ref)
    times = nr.bam_sort_last_times()
    assert times["passes"] == passes and times["scatter_kernel_s"] > 0 and times["histogram_kernel_s"] > 0 and times["scan_kernel_s"] > 0


SORT_COUNTS = (1, 64, 65, 1023, 1024, 1025, 2049)     # one lane, the wavefront's edge, the tile's edge on both sides, a second tile nearly empty
# the digits in which a family's keys differ: no pass; one; two with skipped digits between; an odd number, so the result lies
# in the other buffer; all eight with two values a digit (256 distinct keys at the most), so most keys have equals
KEY_FAMILIES = {"equal": (), "digit_7": (7,), "digits_0_7": (0, 7), "digits_0_3_5": (0, 3, 5), "all_eight_few_values": tuple(range(8))}


def family_keys(family, n):
    """n seeded keys that agree everywhere but in the family's digits"""
    digits = KEY_FAMILIES[family]
    rng = np.random.default_rng([n, sorted(KEY_FAMILIES).index(family)])
    keys = np.full(n, 0x0123456789ABCDEF, np.uint64)
    for d in digits:
        values = rng.choice(256, 2, replace=False) if len(digits) == 8 else np.arange(256)
        drawn = values[rng.integers(0, len(values), n)].astype(np.uint64)
        keys = keys & ~np.uint64(255 << 8 * d) | drawn << np.uint64(8 * d)
    return keys


def passes_of(keys):
    """the digits in which the keys differ: what the sort takes a pass for"""
    differ = int(np.bitwise_and.reduce(keys)) ^ int(np.bitwise_or.reduce(keys))
    return sum(1 for d in range(8) if differ >> (8 * d) & 255)


def key_spans(keys):
    spans = np.zeros(len(keys), nr.BAM_SPAN)            # flags 0: the order is by `key` and by nothing else
    spans["key"] = keys
    return spans


@pytest.mark.parametrize("family", sorted(KEY_FAMILIES))
def test_the_sort_over_arbitrary_keys(hip_device, family):
    """the radix sort as a component: keys that are no BAM record's, every count around a wavefront and a tile"""
    for n in SORT_COUNTS:
        keys = family_keys(family, n)
        passes = passes_of(keys)
        assert passes == (len(KEY_FAMILIES[family]) if n >= 64 else 0), (family, n)
        spans = key_spans(keys)
        perm, bad, _kind = nr.bam_sort_order(spans, device=hip_device)
        assert bad == 0 and nr.bam_sort_last_times()["passes"] == passes, (family, n)
        assert perm.tolist() == np.argsort(keys, kind="stable").tolist(), (family, n)
        assert perm.tobytes() == nr.bam_sort_order(spans)[0].tobytes(), (family, n)


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_one_call_entry(hip_device, huffman):
    for name in B.SORTABLE:
        case = B.CASES[name]
        data, rec_off = stream_of(case)
        members, out_off, member_start, spans, perm, bad, _kind = nr.bam_sorted_bgzf_device(data, rec_off, case.n_ref, True, huffman, hip_device)
        assert bad == 0, name
        order = B.order(case.records, case.n_ref)
        in_order = [case.records[i] for i in order]
        payloads = B.payloads(case.header, in_order)
        want, want_off = nr.bgzf_deflate(payloads, device=hip_device, huffman=huffman)
        assert members.tobytes() == want.tobytes() and out_off.tolist() == want_off.tolist(), name
        assert perm.tolist() == order and member_start.tolist() == np.cumsum([0] + [len(p) for p in payloads]).tolist(), name
        assert H.span_rows(spans) == B.table(len(case.header), in_order, case.n_ref), name
    case = B.CASES["refuse_tid"]
    data, rec_off = stream_of(case)
    assert nr.bam_sorted_bgzf_device(data, rec_off, case.n_ref, True, huffman, hip_device)[5:] == case.refuse[1:]
    case = B.CASES["three_members"]
    data, rec_off = stream_of(case)
    nr.bam_sorted_bgzf_device(data, rec_off, case.n_ref, True, huffman, hip_device)
    times = nr.bam_sort_last_times()
    assert set(times) == {"keys_kernel_s", "histogram_kernel_s", "scan_kernel_s", "scatter_kernel_s", "gather_kernel_s", "total_s", "passes"}
    assert times["keys_kernel_s"] > 0 and times["gather_kernel_s"] > 0 and times["passes"] >= 1
    assert nr.bgzf_deflate_last_times()["deflate_kernel_s"] > 0


def test_times_of_sorted_and_unsorted_calls(hip_device):
    """every kernel of a call is timed between marks of its own, the sort's summed over its passes, and nothing of one call is
    left in the next one's times on the same thread"""
    case = B.CASES["three_members"]
    data, rec_off = stream_of(case)
    sort_kernels = ("histogram_kernel_s", "scan_kernel_s", "scatter_kernel_s")
    assert nr.bam_sorted_bgzf_device(data, rec_off, case.n_ref, True, "fixed", hip_device)[5] == 0
    times = nr.bam_sort_last_times()
    print("sorted", times)
    assert times["keys_kernel_s"] > 0 and times["gather_kernel_s"] > 0 and all(times[k] > 0 for k in sort_kernels) and times["passes"] >= 1
    assert nr.bam_sorted_bgzf_device(data, rec_off, case.n_ref, False, "fixed", hip_device)[5] == 0
    times = nr.bam_sort_last_times()
    print("unsorted", times)
    assert times["keys_kernel_s"] > 0 and times["passes"] == 0
    assert times["gather_kernel_s"] == 0.0 and all(times[k] == 0.0 for k in sort_kernels)


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_writer_on_the_device_writes_the_hosts_files(tmp_path, hip_device, huffman):
    for k, name in enumerate(B.INDEXABLE):
        case = B.CASES[name]
        raw = {}
        for deflate in ("host", "device"):
            path = tmp_path / ("%s%d.bam" % (deflate, k))
            H.write(path, case.header, case.records, sort=True, index="bai", deflate=deflate, huffman=huffman, device=hip_device)
            raw[deflate] = (H.read(path), H.read(str(path) + ".bai"))
        assert raw["device"] == raw["host"], name
        w = B.Written(raw["device"][0])
        assert w.records == [case.records[i] for i in B.order(case.records, case.n_ref)], name
        B.check_structure(B.read_bai(raw["device"][1]), w)


def test_writer_on_the_device_refuses_as_the_host_does(tmp_path, hip_device):
    for name in H.REFUSALS:
        case = B.CASES[name]
        when, number, _kind = case.refuse
        options = dict(index="bai") if when == "order" else dict(sort=True, index="bai")
        errors, files = [], []
        for deflate in ("host", "device"):
            path = tmp_path / ("%s_%s.bam" % (name, deflate))
            with pytest.raises(bam.BamOrderError) as e:
                H.write(path, case.header, case.records, deflate=deflate, device=hip_device, **options)
            errors.append((e.value.record, str(e.value).replace(str(path), "")))
            files.append(H.read(path))
            assert not os.path.exists(str(path) + ".bai")
        assert errors[0] == errors[1] and errors[0][0] == number and files[0] == files[1], name


def no_date(text):
    return [l for l in text.split("\n") if not l.startswith("##fileDate=")]


def check_dump(sorted_path, plain_path):
    """the sorted, indexed dump against the plain one of the same run"""
    w, plain = B.Written(H.read(sorted_path)), B.Written(H.read(plain_path))
    assert len(w.records) > 100 and sorted(w.records) == sorted(plain.records)
    keys = [row[0] for row in w.rows]
    assert keys == sorted(keys) and keys != [row[0] for row in plain.rows]
    assert w.records == [plain.records[i] for i in B.order(plain.records, plain.n_ref)]         # stable
    assert w.text.split("\n")[0].split("\t")[0] == "@HD" and "SO:coordinate" in w.text.split("\n")[0].split("\t")
    assert w.header == B.coordinate_header(plain.header)
    index = B.read_bai(H.read(str(sorted_path) + ".bai"))
    B.check_structure(index, w)
    assert B.check_queries(index, w) >= 200
    f = bam.AlignmentFile(str(sorted_path))
    try:
        tid = f.gettid("2")
        mine = [row for row in w.rows if row[1] == tid and not row[4] & B.UNMAPPED]
        assert len(mine) > 10
        beg, end = mine[len(mine) // 3][2], mine[2 * len(mine) // 3][3]
        # (reads flagged unmapped aside: the reader measures those by their CIGAR, the index gives them one base)
        got = [(r.query_name, r.flag, r.reference_start) for r in f.fetch("2", beg, end) if not r.flag & 4]
        want = [(raw[36:36 + raw[12] - 1].decode("ascii"), int.from_bytes(raw[18:20], "little"), row[2])
                for raw, row in zip(w.records, w.rows) if row[1] == tid and not row[4] & B.UNMAPPED and row[2] < end and row[3] > beg]
        assert want and got == want
    finally:
        f.close()


def test_sv_genotype_python_reader_zlib(tmp_path, hip_device):
    outs = {}
    for label, options in (("plain", {}), ("sorted", dict(alignment_sort=True, alignment_index="bai"))):
        out = str(tmp_path / (label + ".vcf"))
        with open(T.IN_VCF) as inf, open(out, "w") as outf:
            classic.sv_genotype(T.IN_BAM, inf, outf, 20, 1, 1, 1000000, T.LIB_JSON, False, str(tmp_path / (label + ".bam")), None, False, None,
                                1e10, deflate="zlib", **options)
        outs[label] = no_date(open(out).read())
    assert outs["plain"] == outs["sorted"] == no_date(open(T.EXPECTED).read())
    assert not os.path.exists(str(tmp_path / "plain.bam.bai"))
    check_dump(tmp_path / "sorted.bam", tmp_path / "plain.bam")


def test_command_line_sorted_and_indexed_on_the_device(tmp_path, hip_device):
    """`-w ev.bam --sort-alignment --bai --reader device --deflate device` in a child process; and the exit with --bai alone"""
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = [sys.executable, "-m", "svtyper_amd.classic", "-B", T.IN_BAM, "-l", T.LIB_JSON, "-i", T.IN_VCF, "--reader", "device",
              "--deflate", "device"]
    runs = {}
    for label, options in (("plain", []), ("sorted", ["--sort-alignment", "--bai"]), ("bai_alone", ["--bai"])):
        runs[label] = subprocess.run(common + ["-o", str(tmp_path / (label + ".vcf")), "-w", str(tmp_path / (label + ".bam"))] + options,
                                     env=env, cwd=ROOT, capture_output=True, timeout=600)
    assert runs["plain"].returncode == 0 and runs["sorted"].returncode == 0, (runs["plain"].stderr[-2000:], runs["sorted"].stderr[-2000:])
    assert no_date(open(str(tmp_path / "sorted.vcf")).read()) == no_date(open(T.EXPECTED).read())
    check_dump(tmp_path / "sorted.bam", tmp_path / "plain.bam")
    r = runs["bai_alone"]
    assert r.returncode != 0 and b"--sort-alignment" in r.stderr and not os.path.exists(str(tmp_path / "bai_alone.bam.bai"))
    assert H.read(tmp_path / "bai_alone.bam") == H.read(tmp_path / "plain.bam")

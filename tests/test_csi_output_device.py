"""GPU: the CSI fold of the `-w` BAM on the device (svt_bam_index_kernel.h: svt_bam_index_fold_device) against the host fold
(svt_csi_build_bam) byte for byte -- the host fold is itself proven against the plain-Python restatement of tests/csioutcases.py in
tests/test_csi_output_host.py, so this is not the code under test checking itself.  The tables are made here, at the smallest
shapes at which the kernels can go wrong: record counts around a wavefront, a workgroup and a tile of 1 024, runs carried across
tiles, a tail without coordinate that starts on a tile border, a record across members.  Then the writer with deflate="device"."""
import os
import random

import numpy as np
import pytest

import baicases as B
import csioutcases as K
import test_csi_output_host as H
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
TILE = B.TILE
HEADER_LEN = 300


def members_of(lens, header_len=HEADER_LEN):
    """(member_start, member_off) of a header flushed and records handed over one by one, as baicases.payloads cuts them; the file
    offsets are made up (a member takes a third of its payload and 26 bytes)"""
    start, pos, buf = [], 0, header_len

    def emit(l):
        nonlocal pos, buf
        start.append(pos)
        pos += l
        buf -= l
    while buf >= B.PAYLOAD:
        emit(B.PAYLOAD)
    if buf:
        emit(buf)
    for l in lens:
        if buf and buf + l > B.PAYLOAD:
            emit(buf)
        buf += l
        while buf >= B.PAYLOAD:
            emit(B.PAYLOAD)
    if buf:
        emit(buf)
    start.append(pos)
    sizes = np.diff(np.array(start, np.uint64)) // np.uint64(3) + np.uint64(26)
    return np.array(start, np.uint64), np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)


def table(rows, n_ref, lens=None):
    """the span table of records (tid, beg, end, unmapped) in written order, tid -1 for one without coordinate; 60-byte records"""
    n = len(rows)
    spans = np.zeros(n, nr.BAM_SPAN)
    lens = [60] * n if lens is None else lens
    at = HEADER_LEN
    for i, (tid, beg, end, unmapped) in enumerate(rows):
        flags = (nr.BAM_UNMAPPED if unmapped else 0) | (nr.BAM_NO_COOR if tid < 0 else 0) | (nr.BAM_BEYOND if end > 1 << 29 else 0)
        key = (n_ref if tid < 0 else tid) << 33 | ((beg + 1) << 1 if tid >= 0 else 0)
        spans[i] = (at, lens[i], key, tid, beg if tid >= 0 else 0, end if tid >= 0 else 0, flags)
        at += lens[i]
    return spans, lens


def pattern(which, n, spread):
    """(rows, n_ref); `spread`: the distance between neighbours where they lie in bins of their own"""
    if which == "one_bin":                      # one run longer than a tile, carried across tiles
        return [(0, 100, 150, i % 7 == 0) for i in range(n)], 1
    if which == "own_bins":                     # runs == n
        return [(0, i * spread, i * spread + 10, False) for i in range(n)], 1
    if which == "middle_reference_empty":
        first = n // 2
        return [(0, i * 300, i * 300 + 40, i % 5 == 0) for i in range(first)] + [(2, k * 300, k * 300 + 40, k % 5 == 0) for k in range(n - first)], 3
    if which == "long_first_record":            # its end dominates the running maximum across two tile borders
        half = (n + 1) // 2
        rows = []
        for tid, count in ((0, half), (1, n - half)):
            rows += [(tid, 0 if k == 0 else 1000 + k * (spread // 8), 200 * spread if k == 0 else 1000 + k * (spread // 8) + 30, False) for k in range(count)]
        return rows, 2
    if which == "tail_on_a_tile_border":        # the records without coordinate start exactly on one
        placed = n // TILE * TILE if n > TILE else n // 2
        return [(0 if i < placed // 2 else 1, i * 50, i * 50 + 20, i % 3 == 0) for i in range(placed)] + [(-1, 0, 0, True)] * (n - placed), 2
    raise KeyError(which)


def both(spans, n_ref, l_ref_max, start, off, device):
    host = nr.csi_build_bam(spans, n_ref, l_ref_max, start, off)
    got = nr.csi_build_bam(spans, n_ref, l_ref_max, start, off, device=device)
    assert got[1:] == host[1:], (got[1:], host[1:])
    assert got[0] == host[0]
    return got


PATTERNS = ("one_bin", "own_bins", "middle_reference_empty", "long_first_record", "tail_on_a_tile_border")


@pytest.mark.parametrize("l_ref_max", [1 << 29, (1 << 31) - 1])             # depth 5, depth 6
@pytest.mark.parametrize("which", PATTERNS)
def test_device_fold_is_the_host_fold(hip_device, which, l_ref_max):
    depth = nr.csi_depth(l_ref_max)
    assert depth == (5 if l_ref_max == 1 << 29 else 6)
    spread = 1 << 14 if depth == 5 else 1 << 19
    for n in COUNTS:
        rows, n_ref = pattern(which, n, spread)
        assert len(rows) == n
        spans, lens = table(rows, n_ref)
        start, off = members_of(lens)
        csi, bad, _kind = both(spans, n_ref, l_ref_max, start, off, hip_device)
        assert bad == 0 and csi[:4] == b"CSI\1" and csi[8] == depth, (which, n)
        index = K.read_csi(csi)
        assert index["no_coor"] == sum(1 for r in rows if r[0] < 0)
        if which == "own_bins":
            assert sum(len(chunks) for ref in index["refs"] for _l, chunks in ref["bins"].values()) == n
            assert nr.bam_index_last_times()["runs"] == n
        if which == "one_bin" and n:
            assert nr.bam_index_last_times()["runs"] == 1 and nr.bam_index_last_times()["passes"] == 0


def test_a_record_across_members_and_an_end_on_a_member_boundary(hip_device):
    rows = [(0, 10, 60, False), (0, 20, 90, False), (0, 30, 31, False), (0, 1 << 20, (1 << 20) + 5, False), (1, 7, 8, True)]
    lens = [100, 70000, 60560, 80, 90]                  # the second one is cut at 65 280; the third ends where its member ends
    spans, lens = table(rows, 2, lens)
    start, off = members_of(lens)
    assert (start[3] - start[2], start[4] - start[3]) == (B.PAYLOAD, B.PAYLOAD) and int(spans[2]["off"] + spans[2]["len"]) == int(start[4])
    csi, bad, _kind = both(spans, 2, 1 << 29, start, off, hip_device)
    assert bad == 0
    index = K.read_csi(csi)
    (s, e), = index["refs"][0]["bins"][K.reg2bin(10, 90, 5)][1][:1]
    assert s >> 16 == int(off[1]) and e >> 16 == int(off[4]) and e & 0xFFFF == 0        # from the second member to the fifth's first byte


@pytest.mark.parametrize("at", [1, 1024, 1025])
@pytest.mark.parametrize("what", ["tid", "key_back", "beyond", "bad"])
def test_the_first_refused_record_is_the_hosts(hip_device, what, at):
    n = 2049
    rows, n_ref = pattern("own_bins", n, 1 << 14)
    spans, lens = table(rows, 3)
    i = at - 1
    if what == "tid":
        spans[i]["tid"] = 7
    elif what == "key_back":
        if i == 0:
            spans[1]["key"] = 0                         # (the first record has nothing in front: the second one steps back)
            i = 1
        else:
            spans[i]["key"] = spans[i - 1]["key"] - np.uint64(2)
    elif what == "beyond":
        spans[i]["end"] = (1 << 29) + 1
    else:
        spans[i]["flags"] = nr.BAM_BAD | nr.BAM_BAD_POS
    later = min(i + 300, n - 1)                         # a second refusal further on, of another kind: the first one wins
    spans[later]["flags"] = nr.BAM_BAD | nr.BAM_BAD_RECORD
    start, off = members_of(lens)
    csi, bad, kind = both(spans, 3, 1 << 29, start, off, hip_device)
    want = {"tid": nr.BAM_KIND_TID, "key_back": nr.BAM_KIND_KEY_BACK, "beyond": nr.BAM_KIND_BEYOND, "bad": nr.BAM_KIND_POS}[what]
    assert csi is None and (bad, kind) == (i + 1, want)


def test_saturated_end_is_refused_at_depth_6(hip_device):
    rows, n_ref = pattern("own_bins", 70, 1 << 19)
    spans, lens = table(rows, 1)
    spans[69]["end"] = 0xFFFFFFFF
    start, off = members_of(lens)
    assert both(spans, 1, (1 << 31) - 1, start, off, hip_device) == (None, 70, nr.BAM_KIND_BEYOND)
    spans[69]["end"] = 0xFFFFFFFE
    assert both(spans, 1, (1 << 31) - 1, start, off, hip_device)[1] == 0


def passes_of(keys):
    """the digits in which the keys differ: what a radix sort of them takes a pass for (as bamfirstcases.radix_passes for hashes)"""
    keys = [int(k) for k in keys]
    differ = 0
    for k in keys:
        differ |= k ^ keys[0]
    return sum(1 for d in range(8) if differ >> (8 * d) & 255)


def test_two_sorts_in_one_call_keep_their_own_times(hip_device):
    """svt_bam_sorted_bgzf_csi_device sorts twice on one thread: the records by key and, in the fold behind the members, the runs by
    tid << 32 | bin.  Here the two take pass counts of different parity -- the record keys (pos + 1) << 1 of pos = 16384 w differ in
    digits 1 and 2, the leaf bins 4681 + w in digit 0 alone --, so each result lies in another of its sort's two buffers, and each
    sort's passes and seconds are its own call's."""
    rnd = random.Random(7)
    ws = list(range(182)) + [rnd.randrange(182) for _ in range(1025 - 182)]
    rnd.shuffle(ws)
    case = K.Case([B.rec("r%d" % i, 0, 16384 * w, 0, K._m(20)) for i, w in enumerate(ws)], [K.D5])
    sort_kernels = ("histogram_kernel_s", "scan_kernel_s", "scatter_kernel_s")

    def stream(records):
        rec_off = np.cumsum([len(case.header)] + [len(r) for r in records]).astype(np.uint64)
        return case.header + b"".join(records), rec_off

    def host_route(records, sort):
        """(members, out_off, the .csi, the span table as written) of the host's entries"""
        data, rec_off = stream(records)
        spans = nr.bam_spans(data, rec_off, case.n_ref)[0]
        perm = nr.bam_sort_order(spans)[0] if sort else np.arange(len(records), dtype=np.uint64)
        written = spans[perm]
        written["off"] = np.cumsum(written["len"]) - written["len"] + np.uint64(len(case.header))
        payloads = B.payloads(case.header, [records[i] for i in perm.tolist()])
        members, out_off = nr.bgzf_deflate(payloads)
        start = np.cumsum([0] + [len(p) for p in payloads]).astype(np.uint64)
        csi, bad, _kind = nr.csi_build_bam(written, case.n_ref, K.D5, start, out_off)
        assert bad == 0
        return members, out_off, csi, written, spans

    members, out_off, csi, written, spans = host_route(case.records, True)
    bins = [K.reg2bin(int(r["beg"]), max(int(r["end"]), int(r["beg"]) + 1), 5) for r in written]
    record_passes, run_passes = passes_of(spans["key"]), passes_of([int(r["tid"]) << 32 | b for r, b in zip(written, bins)])
    assert (record_passes, run_passes) == (2, 1) and sorted(set(bins)) == list(range(4681, 4681 + 182))
    data, rec_off = stream(case.records)
    got = nr.bam_sorted_bgzf_csi_device(data, rec_off, case.n_ref, K.D5, True, "fixed", hip_device)
    assert got[6:] == (0, 0, 0, 0)
    assert got[0].tobytes() == members.tobytes() and got[1].tolist() == out_off.tolist() and got[5] == csi
    assert got[3].tobytes() == written.tobytes()
    sort_times, index_times = nr.bam_sort_last_times(), nr.bam_index_last_times()
    print("record sort", sort_times, "fold", index_times)
    assert sort_times["passes"] == record_passes and all(sort_times[k] > 0 for k in sort_kernels)
    assert index_times["passes"] == run_passes and index_times["sort_kernel_s"] > 0 and index_times["runs"] == len(set(bins))
    # the same records in order already, written as they come: no record sort, the fold's sort as before
    in_order = [case.records[i] for i in got[4].tolist()]
    members, out_off, csi, written, _spans = host_route(in_order, False)
    data, rec_off = stream(in_order)
    got = nr.bam_sorted_bgzf_csi_device(data, rec_off, case.n_ref, K.D5, False, "fixed", hip_device)
    assert got[6:] == (0, 0, 0, 0)
    assert got[0].tobytes() == members.tobytes() and got[1].tolist() == out_off.tolist() and got[5] == csi
    sort_times = nr.bam_sort_last_times()
    assert sort_times["passes"] == 0 and all(sort_times[k] == 0.0 for k in sort_kernels)
    assert nr.bam_index_last_times()["passes"] == run_passes and nr.bam_index_last_times()["runs"] == len(set(bins))


WRITTEN = [("bai", "three_members"), ("bai", "long_record"), ("bai", "member_edge_last"), ("bai", "n1025"), ("csi", "far"), ("csi", "running_maximum"),
           ("csi", "only_no_coordinate"), ("csi", "header_only"), ("csi", "leaf_edges_depth5")]


@pytest.mark.parametrize("huffman", ["fixed", "dynamic"])
def test_the_writer_with_the_device_fold(hip_device, tmp_path, huffman):
    for corpus, name in WRITTEN:
        case = (B.CASES if corpus == "bai" else K.CASES)[name]
        for sort in (True, False):
            records = case.records if sort else [case.records[i] for i in B.order(case.records, case.n_ref)]
            options = dict(sort=sort, index="bai", huffman=huffman, device=hip_device)
            H.write(tmp_path / "device.bam", case.header, records, csi=True, deflate="device", **options)
            H.write(tmp_path / "host.bam", case.header, records, csi=True, deflate="host", **options)
            H.write(tmp_path / "plain.bam", case.header, records, deflate="device", sort=sort, huffman=huffman, device=hip_device)     # no index at all
            assert H.read(tmp_path / "device.bam") == H.read(tmp_path / "plain.bam") == H.read(tmp_path / "host.bam"), (name, sort)
            assert K.inflate(H.read(tmp_path / "device.bam.csi")) == K.inflate(H.read(tmp_path / "host.bam.csi")), (name, sort)
            assert K.inflate(H.read(tmp_path / "device.bam.csi")) == K.build_csi_bam(B.Written(H.read(tmp_path / "device.bam"))), (name, sort)
            assert not os.path.exists(str(tmp_path / "device.bam.bai"))


def test_the_writer_reports_what_the_device_fold_refuses(hip_device, tmp_path):
    for name in K.REFUSED:
        case = K.CASES[name]
        with pytest.raises(H.bam.BamOrderError) as e:
            H.write(tmp_path / "ev.bam", case.header, case.records, sort=True, index="bai", csi=True, deflate="device", device=hip_device)
        assert e.value.record == case.refuse[0] and not os.path.exists(str(tmp_path / "ev.bam.csi"))
        assert B.Written(H.read(tmp_path / "ev.bam")).records == [case.records[i] for i in B.order(case.records, case.n_ref)]
    case = B.CASES["unsorted_bai_alone"]
    with pytest.raises(H.bam.BamOrderError) as e:
        H.write(tmp_path / "u.bam", case.header, case.records, index="bai", csi=True, deflate="device", device=hip_device)
    assert e.value.record == case.refuse[1] and not os.path.exists(str(tmp_path / "u.bam.csi"))

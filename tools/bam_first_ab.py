#!/usr/bin/env python
"""What "first occurrences of a record stream" costs, in ONE process, interleaved -- the pass rank 0 runs over the gathered dumps
of a sharded `svtyper -w --gather-alignment` run (svtyper_amd/sharded.py):
  python_set_loop   driver._write_dumped over the whole stream with a writer that does nothing: the (query_name, flag) `set` and
                    the per-record Python loop, which is what de-duplicates a dump today -- the baseline
  host_entry        native_reads.bam_first(data, rec_off)                  svt_bam_first_host: a hash set of views
  device_entry      native_reads.bam_first(data, rec_off, device=...)      svt_bam_first_device, wall: upload, kernels, keep down
  device_kernels    its kernels by HIP events (svt_bam_first_last_times)
and the whole rank-0 tail, from the end of the gather to the end of close() (sharded._write_gathered: the pass, the writer opened
with --sort-alignment --alignment-csi, write_raw_many, close()), for --deflate device and --deflate host.  Inputs:
  twice     the fixture's dump (reader="device" into a bam.RecordSink) taken twice, as two ranks that met the same reads would hand
            it over: half the records are duplicates;
  twice_x   --copies (default 25) copies of the dump, a copy's reads renamed by its number, and all of them again: 50 times the
            fixture's dump, half of it duplicates.
--reps timed runs (default 5; the tails of twice_x: --tail-reps, default 1) after one untimed run each.  The three answers are
compared on the untimed runs.  Prints one JSON object and, with --out FILE, writes it there.  GPU box only."""
import io
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svtyper_amd import bam, classic, driver, sharded  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, tail_reps, copies, out_path, device = arg("--reps", 5), arg("--tail-reps", 1), arg("--copies", 25), arg("--out", ""), arg("--device", 0)
data_dir = os.path.join(ROOT, "tests", "data")
IN_BAM = os.path.join(data_dir, "NA12878.target_loci.sorted.bam")


def dump():
    """the records of the fixture's `-w` dump, one bytes each"""
    class Sink(io.StringIO):
        def close(self):
            pass
    sink = bam.RecordSink()
    with open(os.path.join(data_dir, "example.vcf")) as vcf:
        classic.sv_genotype(IN_BAM, vcf, Sink(), 20, 1, 1, 1000000, os.path.join(data_dir, "NA12878.bam.json"), False, None, None, False, None,
                            1e10, reader="device", alignment_out=sink)
    return [bytes(sink.data[a:b]) for a, b in zip(sink.offsets, sink.offsets[1:])]


def renamed(records, k):
    """copy k of the records: its reads' names with the copy's number in front (block_size and l_read_name follow)"""
    out, tag = [], b"%02d" % k
    for raw in records:
        size, l_read_name = struct.unpack_from("<i", raw, 0)[0], raw[12]
        assert l_read_name + 2 <= 255
        out.append(struct.pack("<i", size + 2) + raw[4:12] + bytes([l_read_name + 2]) + raw[13:36] + tag + raw[36:])
    return out


class Nowhere:
    """the writer of the baseline: what would be written is counted, nothing else"""
    def __init__(self):
        self.kept = []

    def write_raw(self, record):
        self.kept.append(len(record))


class Engine:
    def __init__(self, device):
        self.device = device


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def stat(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


result = {"reps": reps, "tail_reps": tail_reps, "copies": copies, "device": device}
fixture = dump()
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "ev.bam")
    for name, half, n_tail in (("twice", fixture, reps), ("twice_x", [raw for k in range(copies) for raw in renamed(fixture, k)], tail_reps)):
        records = half + half
        del half
        data = b"".join(records)
        lens = np.array([len(r) for r in records], np.uint32)
        del records
        n = int(lens.shape[0])
        rec_off = np.concatenate((np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)))
        entry = {"records": n, "record_bytes": len(data)}
        array = np.frombuffer(data, np.uint8)

        def tail(deflate):
            return sharded._write_gathered((array, lens, [n // 2, n - n // 2]), path, IN_BAM,
                                           dict(deflate=deflate, alignment_sort=True, alignment_index="csi", engine=Engine(device)))
        # untimed: the library and the kernels loaded, and the three answers compared
        nowhere = Nowhere()
        driver._write_dumped(data, nowhere, set())
        host, _ = nr.bam_first(data, rec_off)
        dev, _ = nr.bam_first(data, rec_off, device=device)
        entry["kept"] = int(host.sum())
        entry["answers_agree"] = bool(np.array_equal(host, dev) and lens[host.astype(bool)].tolist() == nowhere.kept and entry["kept"] * 2 == n)
        files = {}
        for deflate in ("device", "host"):
            counts = tail(deflate)
            files[deflate] = (open(path, "rb").read(), open(path + ".csi", "rb").read())
            entry["answers_agree"] = entry["answers_agree"] and counts["kept"] == entry["kept"]
        entry["device_tail_equals_host_tail"] = files["device"] == files["host"]
        del files
        walls = {k: [] for k in ("python_set_loop_ms", "host_entry_ms", "device_entry_ms")}
        kernels = []
        for _ in range(reps):
            walls["python_set_loop_ms"].append(timed(lambda: driver._write_dumped(data, Nowhere(), set()))[0])
            walls["host_entry_ms"].append(timed(lambda: nr.bam_first(data, rec_off))[0])
            walls["device_entry_ms"].append(timed(lambda: nr.bam_first(data, rec_off, device=device))[0])
            kernels.append(nr.bam_first_last_times())
        tails = {"device": [], "host": []}
        for _ in range(n_tail):
            for deflate in tails:
                tails[deflate].append(timed(lambda: tail(deflate))[0])
        entry.update({k: stat(v) for k, v in walls.items()})
        entry["device_kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0] if k.endswith("kernel_s")}
        entry["device_kernels_ms_median"]["sum_ms"] = sum(entry["device_kernels_ms_median"].values())
        entry["device_passes"] = kernels[0]["passes"]
        entry["rank0_tail_ms"] = {deflate: stat(v) for deflate, v in tails.items()}
        entry["python_set_loop_over_host_entry"] = entry["python_set_loop_ms"]["median"] / entry["host_entry_ms"]["median"]
        entry["python_set_loop_over_device_entry"] = entry["python_set_loop_ms"]["median"] / entry["device_entry_ms"]["median"]
        entry["host_entry_over_device_entry"] = entry["host_entry_ms"]["median"] / entry["device_entry_ms"]["median"]
        result[name] = entry
        print(name, json.dumps(entry), flush=True)
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

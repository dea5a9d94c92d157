#!/usr/bin/env python
"""What --sort-alignment and --bai cost at close(), in ONE process, interleaved: bam.AlignmentFile(path, "wb", ...) per deflate
choice (zlib, host, device) in three modes --
  plain        no option: the writer as it was, the baseline (its wall time is write_raw() of every record and close())
  sort         sort=True over the records as the drivers write them
  sort_index   sort=True, index="bai"
-- from the first write_raw() to the end of close().  --reps timed runs (default 5) after one untimed run each.  Inputs:
  bam      the records of the `-w` BAM that tools/deflate_ab.py's workload writes (the fixture's variant lines x --times,
           reader="device"; the run-wide de-duplication keeps it the fixture's dump);
  bam_x    the same records --copies times (default 50), a copy's positions moved by its number: the size at which the kernels
           are more than their launches.
For the device legs the kernels' own times from HIP events: the keys, sort and gather kernels (svt_bam_sort_last_times) beside
the deflate kernels of the same call (svt_bgzf_deflate_last_times); and `host_stable_sort`: std::stable_sort of the same keys
(svt_bam_sort_order_host) beside the device sort (svt_bam_sort_order_device, wall and kernels).  Every sorted file is checked
against the checker of tests/baicases.py once, on the untimed runs, and device files with host files.  Prints one JSON object
and, with --out FILE, writes it there.  GPU box only.  --deflate device (a comma-separated choice of zlib,host,device; default
all three) times those legs alone; with --package-root DIR (without --plain-only: a checkout that has the options) that is how
one commit is measured against another in one session (profiles/held_close_ab.json).

The plain legs are the code path of the commit before the options, and profiles/bam_sort_ab.json keeps them re-measured on that
commit under `parent_commit_plain`.  Two commands make the file, PARENT being a built checkout of that commit:
    python tools/bam_sort_ab.py --plain-only --package-root PARENT --out parent_plain.json
    python tools/bam_sort_ab.py --merge-parent parent_plain.json --out profiles/bam_sort_ab.json"""
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
# --package-root DIR --plain-only: the plain legs alone over the svtyper_amd of another checkout (one from before the options)
sys.path.insert(0, sys.argv[sys.argv.index("--package-root") + 1] if "--package-root" in sys.argv else ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import baicases as B  # noqa: E402
from svtyper_amd import bam, classic  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, copies, out_path, device = arg("--reps", 5), arg("--times", 20), arg("--copies", 50), arg("--out", ""), arg("--device", 0)
data = os.path.join(ROOT, "tests", "data")
DEFLATES = tuple(arg("--deflate", "zlib,host,device").split(","))
IN_BAM = os.path.join(data, "NA12878.target_loci.sorted.bam")


def dump():
    """(the template, the records) of the `-w` BAM of tools/deflate_ab.py's workload"""
    class Sink(io.StringIO):
        def close(self):
            pass
    lines = open(os.path.join(data, "example.vcf")).readlines()
    text = "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * times)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.bam")
        classic.sv_genotype(IN_BAM, io.StringIO(text), Sink(), 20, 1, 1, 1000000, os.path.join(data, "NA12878.bam.json"), False, path, None,
                            False, None, 1e10, reader="device")
        w = B.Written(open(path, "rb").read())
    template = bam.AlignmentFile(IN_BAM, "rb")
    return template, w.records


def moved(records, k):
    out = []
    for raw in records:
        tid, pos = struct.unpack_from("<ii", raw, 4)
        out.append(raw if tid < 0 or k == 0 else raw[:8] + struct.pack("<i", pos + 37 * k) + raw[12:])
    return out


def close_time(path, template, records, **options):
    t0 = time.perf_counter()
    out = bam.AlignmentFile(path, "wb", template=template, device=device, **options)
    for raw in records:
        out.write_raw(raw)
    out.close()
    return time.perf_counter() - t0


MODES = {"plain": {}, "sort": {"sort": True}, "sort_index": {"sort": True, "index": "bai"}}
plain_only = "--plain-only" in sys.argv
if plain_only:
    MODES = {"plain": {}}
result = {"reps": reps, "times": times, "copies": copies, "device": device, "package": "another checkout (--package-root)" if "--package-root" in sys.argv else "this checkout", "plain_only": plain_only, "deflates": list(DEFLATES)}
template, fixture = dump()
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "ev.bam")
    for name, records in (("bam", fixture), ("bam_x", [raw for k in range(copies) for raw in moved(fixture, k)])):
        entry = {"records": len(records), "record_bytes": sum(len(r) for r in records)}
        legs = [(deflate, mode) for deflate in DEFLATES for mode in MODES]
        files, ok = {}, True
        n_ref = len(template.references)
        order = B.order(records, n_ref)
        for deflate, mode in legs:                                     # untimed: the library loaded, the kernels loaded
            close_time(path, template, records, deflate=deflate, **MODES[mode])
            files[deflate, mode] = (open(path, "rb").read(), open(path + ".bai", "rb").read() if mode == "sort_index" else None)
            w = B.Written(files[deflate, mode][0])
            ok = ok and w.records == (records if mode == "plain" else [records[i] for i in order])
            if mode == "sort_index":
                B.check_structure(B.read_bai(files[deflate, mode][1]), w)
        entry["records_and_structure"] = ok
        if "device" in DEFLATES and "host" in DEFLATES:
            entry["device_equals_host"] = all(files["device", mode] == files["host", mode] for mode in MODES)
        walls = {leg: [] for leg in legs}
        kernels, sorts = [], {"host_stable_sort_ms": [], "device_sort_wall_ms": [], "device_sort_kernels_ms": []}
        rec_off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
        spans = None if plain_only else nr.bam_spans(b"".join(records), rec_off, n_ref)[0]
        for _ in range(reps):
            for deflate, mode in legs:
                walls[deflate, mode].append(close_time(path, template, records, deflate=deflate, **MODES[mode]) * 1e3)
                if (deflate, mode) == ("device", "sort_index"):
                    kernels.append(dict(nr.bam_sort_last_times(), **{"deflate_" + k: v for k, v in nr.bgzf_deflate_last_times().items()}))
            if plain_only:
                continue
            t0 = time.perf_counter()
            nr.bam_sort_order(spans)
            sorts["host_stable_sort_ms"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            nr.bam_sort_order(spans, device=device)
            sorts["device_sort_wall_ms"].append((time.perf_counter() - t0) * 1e3)
            t = nr.bam_sort_last_times()
            sorts["device_sort_kernels_ms"].append((t["histogram_kernel_s"] + t["scan_kernel_s"] + t["scatter_kernel_s"]) * 1e3)
        for deflate in DEFLATES:
            entry[deflate] = {mode: {"wall_ms_median": statistics.median(walls[deflate, mode]), "wall_ms_min": min(walls[deflate, mode]),
                                     "wall_ms_max": max(walls[deflate, mode])} for mode in MODES}
            if plain_only:
                continue
            base = entry[deflate]["plain"]["wall_ms_median"]
            entry[deflate]["sort_over_plain"] = entry[deflate]["sort"]["wall_ms_median"] / base
            entry[deflate]["sort_index_over_plain"] = entry[deflate]["sort_index"]["wall_ms_median"] / base
        result[name] = entry
        if plain_only or "device" not in DEFLATES:
            continue
        entry["sort_alone"] = {k: {"median": statistics.median(v), "min": min(v)} for k, v in sorts.items()}
        entry["device"]["passes"] = kernels[0]["passes"]
        entry["device"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0] if k.endswith("kernel_s")}
        new_ms = sum(v for k, v in entry["device"]["kernels_ms_median"].items() if not k.startswith("deflate_"))
        entry["device"]["new_kernels_over_deflate_kernel"] = new_ms / entry["device"]["kernels_ms_median"]["deflate_deflate_kernel_ms"]
        result[name] = entry
template.close()
if "--merge-parent" in sys.argv:        # the --plain-only --package-root run's JSON, kept beside this run's figures
    with open(sys.argv[sys.argv.index("--merge-parent") + 1]) as f:
        parent = json.load(f)
    result["parent_commit_plain"] = {k: parent[k] for k in ("reps", "times", "copies", "bam", "bam_x")}
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

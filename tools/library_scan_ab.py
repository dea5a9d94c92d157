#!/usr/bin/env python
"""A/B/C of the library scan in ONE process on the same inputs, interleaved (a, b, c, a, b, c, ...):
  host            svt_bam_scan_library summed over the file's libraries (three passes per library on one host thread)
  device          svt_bam_scan_libraries_device, members inflated by host threads, the arena uploaded
  device_inflate  svt_bam_scan_libraries_device, compressed members uploaded, svt_inflate_kernel writes the arena
on the fixture BAM and on a 30x whole-genome-like synthetic BAM of at least --pairs qualifying pairs (bench._wgs_like_bam, the
kind tools/driver_e2e.py builds), with -n 1 000 000.  Per route: wall time (median and range over --reps runs after one untimed
run each) and, for the device routes, the stage split of svt_library_scan_stats of the last run.  Writes one JSON object to
--out (default profiles/library_scan_ab.json) and prints it.  GPU box only."""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from svtyper_amd import native_reads  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps = int(arg("--reps", 5))
pairs = int(arg("--pairs", 1_020_000))
out_path = arg("--out", os.path.join(ROOT, "profiles", "library_scan_ab.json"))
NUM_SAMP = 1_000_000
ROUTES = ("host", "device", "device_inflate")


def groups_of(bam):
    names = []
    for rg in bam.header["RG"]:
        if rg.get("LB", "") not in names:
            names.append(rg.get("LB", ""))
    return [[rg["ID"] for rg in bam.header["RG"] if rg.get("LB", "") == n] for n in names]


def run(bam, groups, route):
    if route == "host":
        return [(r[0], list(r[1].items()), r[2], r[3]) for r in (bam.scan_library(g, NUM_SAMP) for g in groups)], None
    res = bam.scan_libraries(groups, NUM_SAMP, route="device", inflate="device" if route == "device_inflate" else "host", ordered=True)
    return res, dict(bam.library_scan_stats)


def measure(path):
    bam = native_reads.NativeBam(path)
    groups = groups_of(bam)
    first = {r: run(bam, groups, r)[0] for r in ROUTES}          # untimed: first touch of the file, kernels loaded
    out = {"bam_bytes": os.path.getsize(path), "libraries": len(groups), "num_samp": NUM_SAMP,
           "same_result": first["host"] == first["device"] == first["device_inflate"],
           "qualifying_reads": [sum(c for _, c in lib[1]) for lib in first["host"]]}
    walls = {r: [] for r in ROUTES}
    stats = {}
    for _ in range(reps):
        for r in ROUTES:
            t0 = time.perf_counter()
            _, st = run(bam, groups, r)
            walls[r].append(time.perf_counter() - t0)
            if st:
                stats[r] = st
    for r in ROUTES:
        out[r] = {"wall_s_median": statistics.median(walls[r]), "wall_s_min": min(walls[r]), "wall_s_max": max(walls[r])}
        if r in stats:
            out[r]["stats"] = stats[r]
    for r in ROUTES[1:]:
        out["host_over_" + r] = out["host"]["wall_s_median"] / out[r]["wall_s_median"]
    bam.close()
    return out


result = {"reps": reps, "stamp": bench.library_stamp(), "cpu": bench.cpu_model()}
result["fixture"] = measure(os.path.join(ROOT, "tests", "data", "NA12878.target_loci.sorted.bam"))
print(json.dumps({"fixture": result["fixture"]}), flush=True)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "wgs.bam")
    t0 = time.perf_counter()
    _, _, n_records = bench._wgs_like_bam(path, genome=pairs * 10, seed=7)
    print("built %s: %d records in %.0f s" % (path, n_records, time.perf_counter() - t0), flush=True)
    result["wgs_like_30x"] = dict(measure(path), records=n_records)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(result, indent=1, sort_keys=True))

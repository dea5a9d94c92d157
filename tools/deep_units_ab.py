#!/usr/bin/env python
"""Deep units (more than 1 024 kept reads each) through the reader stage, A/B in ONE process on one input, routes interleaved
(native, device, native, device, ...) after one untimed call each: median and range of the wall time over --reps calls.
  native : svt_bam_evidence on the host + svt_batch_create of its records (what reader="native" hands the genotype pass)
  device : svt_bam_evidence_device (reader="device"): the resident batch built on the GPU
The input is --units sites of --reads kept reads each in one BAM written by tests/bamwriter.py (names pair up, a tenth of the
reads carries a split alignment).  --package-root DIR imports svtyper_amd from DIR instead of this tree: with a build of the
parent commit there, `device` is the route in which every deep unit is the host reader's (the figure this change is compared
with comes from that build, never from the tree under test).  Prints one JSON object.  GPU box only.

--parent-root DIR makes the three-route comparison of profiles/deep_units_ab.json in one command: the tool runs itself in two
fresh processes, one after the other, first over the build in DIR and then over this tree (two builds of one package cannot
share a process), each with its own two routes interleaved, and prints
  a_native                : reader="native", from the process of THIS tree (the parent's process reports its own beside (b))
  b_device_parent_commit  : reader="device" of the build in DIR
  c_device_this_change    : reader="device" of this tree
with c_over_b and c_over_a from the medians:
  python tools/deep_units_ab.py --parent-root DIR > profiles/deep_units_ab.json"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def compare_with_parent(parent_root):
    """both builds, a fresh process each; the combined object"""
    passed = [x for k in ("--reps", "--units", "--reads", "--inflate") if k in sys.argv for x in (k, sys.argv[sys.argv.index(k) + 1])]
    runs = {}
    for name, root in (("parent", os.path.abspath(parent_root)), ("change", ROOT)):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--package-root", root] + passed, check=True, stdout=subprocess.PIPE, text=True).stdout
        runs[name] = json.loads(out.strip().split("\n")[-1])
    parent, change = runs["parent"], runs["change"]

    def device(r):
        d = {"wall_s": r["wall_s"]["device"], "native_wall_s_same_process": r["wall_s"]["native"], "units_host": r["device_units_host"],
             "units_host_by_reason": r["device_units_host_by_reason"], "stages_median_s": r["device_stages_median_s"]}
        if "deep" in r:
            d["deep"] = r["deep"]
        return d

    b, c, a = device(parent), device(change), change["wall_s"]["native"]
    print(json.dumps({
        "tool": "tools/deep_units_ab.py --parent-root <build of the parent commit> " + " ".join(passed),
        "processes": "two, one after the other: the parent's build, then this tree; in each, native and device interleaved after an untimed call each",
        "input": {k: change[k] for k in ("units", "kept_reads_per_unit", "records", "reps", "inflate")},
        "a_native": dict(a, process="this change"),
        "b_device_parent_commit": b,
        "c_device_this_change": c,
        "same_bytes": parent["same_bytes"] and change["same_bytes"] and parent["records"] == change["records"],
        "c_over_b": c["wall_s"]["median"] / b["wall_s"]["median"],
        "c_over_a": c["wall_s"]["median"] / a["median"],
    }, indent=1))


if "--parent-root" in sys.argv:
    compare_with_parent(arg("--parent-root", ""))
    sys.exit(0)

package_root = os.path.abspath(arg("--package-root", ROOT))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, package_root)
import numpy as np  # noqa: E402
import walkcases as W  # noqa: E402
from svtyper_amd import evidence as ev, hip, native_reads as nr  # noqa: E402

reps, n_units, n_reads, inflate = arg("--reps", 5), arg("--units", 48), arg("--reads", 9000), arg("--inflate", "host")


def build_input(tmp):
    import bamwriter as bw
    length = 2000 * n_units + 100_000
    header = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:%d\n@RG\tID:rg\tSM:s\tLB:lib\n" % length
    rg = ("RG", "Z", "rg")
    records, sites = [], []
    for s in range(n_units):
        at = 10_000 + 2000 * s
        sites.append({"breakpoint": {"id": "s%d" % s, "svtype": "DEL", "var_length": 800,
                                     "A": {"chrom": "1", "pos": at + 50, "ci": [0, 0], "is_reverse": False},
                                     "B": {"chrom": "1", "pos": at + 851, "ci": [0, 0], "is_reverse": True}}})
        for k in range(n_reads):
            split = k % 10 == 3
            r = W._read("s%dq%05d" % (s, (k * 7919) % (n_reads // 2 + 17)), at + k % 90, cigar="60M40S" if split else "100M",
                        tags=[rg, ("SA", "Z", "1,%d,+,60S40M,60,0;" % (at + 801))] if split else None,
                        flag=0x1 | (0x40 if k % 2 else 0x80) | (0x10 if k % 5 == 0 else 0))
            r["mpos"] = at + 300
            records.append(r)
    path = os.path.join(tmp, "deep_ab.bam")
    bw.write_bam(path, header, [("1", length)], sorted(records, key=lambda r: r["pos"]))
    sample, nbam = W.open_sample(path, W.INFO)
    return sites, sample, nbam


def main():
    with tempfile.TemporaryDirectory() as tmp:
        sites, sample, nbam = build_input(tmp)
        a = W.unit_arrays(sites, sample, nbam, nr.COUNT_CLASSIC)
        head = W.header_batch(sample, a[1])

        def native():
            off, recs, skipped = nbam.evidence(a[0], a[1], a[2], a[3], None, nr.COUNT_CLASSIC, a[4], 20, 3, 0)
            units = head.units.copy()
            units["flags"] = np.where(skipped != 0, ev.UNIT_SKIP, 0)
            d = hip.DeviceBatch(ev.EvidenceBatch(off, units, recs, head.libs, 1.0, 1.0), 0, 0)
            out = nr.batch_records(d)[1].tobytes() if check else None
            d.close()
            return out, {}

        def device():
            kw = {"inflate": inflate} if inflate != "host" else {}
            d, _skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], None, nr.COUNT_CLASSIC, a[4], 20, 3, head, 0, 0, 0, **kw)
            out = nr.batch_records(d)[1].tobytes() if check else None
            d.close()
            return out, stats

        routes = (("native", native), ("device", device))
        check = True
        first = {name: run() for name, run in routes}            # untimed: files touched, kernels loaded, bytes compared
        check = False
        walls = {name: [] for name, _ in routes}
        stages = []
        for _ in range(reps):
            for name, run in routes:
                t0 = time.perf_counter()
                _, stats = run()
                walls[name].append(time.perf_counter() - t0)
                if name == "device":
                    stages.append(stats)
        med = lambda xs: statistics.median(xs)
        result = {
            "package_root": os.path.relpath(package_root, ROOT), "units": n_units, "kept_reads_per_unit": n_reads, "reps": reps, "inflate": inflate,
            "same_bytes": first["native"][0] == first["device"][0], "records": len(first["native"][0]) // 16,
            "wall_s": {name: {"median": med(w), "min": min(w), "max": max(w)} for name, w in walls.items()},
            "device_over_native": med(walls["device"]) / med(walls["native"]),
            "device_units_host": first["device"][1]["units_host"], "device_units_host_by_reason": first["device"][1]["units_host_by_reason"],
            "device_stages_median_s": {k: med([s[k] for s in stages]) for k in ("host_arena_s", "upload_s", "device_walk_s", "host_fallback_s", "batch_create_s")},
        }
        if "deep" in first["device"][1]:
            result["deep"] = dict(first["device"][1]["deep"], deep_walk_s=med([s["deep"]["deep_walk_s"] for s in stages]))
        print(json.dumps(result))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""A/B/C of reader="native", reader="device" and reader="device" + inflate="device" (route name "device_inflate") in ONE process
on the same inputs, interleaved (a, b, c, a, b, c, ...): the
`driver_sso` input (the fixture's 212 variant lines x 100) and the `driver_classic_8bam` input (8 whole-genome-like BAMs x
10 530 DEL lines) that bench.py's real_data legs construct.  Per route: wall time (median and range over --reps runs after one
untimed run each), process CPU seconds per unit, and for the device route the stage split svt_bam_evidence_device reports
(host arena = BAI lookup + inflate, upload, device walk, host fallback, batch create) summed over the run's calls; for the
device-inflate route also svt_evidence_inflate_stats (host index, compressed upload, inflate kernel, blocks inflated against the
blocks the host-inflate route touches: SVT_COUNT_HOST_BLOCKS=1 is set for the untimed run only).  Prints one JSON object.
GPU box only."""
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from svtyper_amd import classic, singlesample  # noqa: E402

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
data = os.path.join(ROOT, "tests", "data")
lines = open(os.path.join(data, "example.vcf")).readlines()
head = [l for l in lines if l.startswith("#")]
body = [l for l in lines if not l.startswith("#")]


class Sink(io.StringIO):
    def close(self):
        pass


ROUTES = ("native", "device", "device_inflate")


def route_kw(route):
    return dict(reader="device", inflate="device") if route == "device_inflate" else dict(reader=route)


def measure(run, n_units):
    out = {}
    texts = {}
    first = {}
    for reader in ROUTES:
        os.environ["SVT_COUNT_HOST_BLOCKS"] = "1"
        first[reader] = {}
        texts[reader] = run(reader, first[reader])  # untimed: first touch of the files, kernels loaded
        os.environ["SVT_COUNT_HOST_BLOCKS"] = "0"
    out["same_bytes"] = texts["native"] == texts["device"] == texts["device_inflate"]
    walls = {r: [] for r in ROUTES}
    cpus = {r: [] for r in ROUTES}
    stages, stages_inflate = [], []
    for _ in range(reps):
        for reader in ROUTES:
            stats = {}
            c0, t0 = time.process_time(), time.perf_counter()
            run(reader, stats)
            walls[reader].append((time.perf_counter() - t0) * 1e3)
            cpus[reader].append((time.process_time() - c0) / n_units * 1e6)
            if reader == "device":
                stages.append(stats["device_reader"])
            if reader == "device_inflate":
                stages_inflate.append(stats["device_reader"])
    for reader in walls:
        w = sorted(walls[reader])
        out[reader] = {"wall_ms_median": statistics.median(w), "wall_ms_min": w[0], "wall_ms_max": w[-1],
                       "cpu_us_per_unit_median": statistics.median(cpus[reader]), "units_per_s_median": n_units / statistics.median(w) * 1e3}
    last = stages[-1]
    out["device_stage_ms"] = {k[:-2]: statistics.median(s[k] for s in stages) * 1e3 for k in last if k.endswith("_s")}
    out["device_counters"] = {k: last[k] for k in last if not k.endswith("_s")}
    last = stages_inflate[-1]
    out["device_inflate_stage_ms"] = {k[:-2]: statistics.median(s[k] for s in stages_inflate) * 1e3 for k in last if k.endswith("_s")}
    out["device_inflate_stage_ms"].update({"inflate." + k[:-2]: statistics.median(s["inflate"][k] for s in stages_inflate) * 1e3
                                           for k in last["inflate"] if k.endswith("_s")})
    out["device_inflate_counters"] = {k: last[k] for k in last if not k.endswith("_s") and k != "inflate"}
    out["device_inflate_counters"]["inflate"] = {k: v for k, v in first["device_inflate"]["device_reader"]["inflate"].items() if not k.endswith("_s")}
    out["device_inflate_vs_device_wall_ms"] = out["device_inflate"]["wall_ms_median"] - out["device"]["wall_ms_median"]
    native_range = out["native"]["wall_ms_max"] - out["native"]["wall_ms_min"]
    gain = out["native"]["wall_ms_median"] - out["device"]["wall_ms_median"]
    out["verdict"] = ("device faster than native by more than native's own range" if gain > native_range else
                      "device slower than native" if gain < 0 else "device faster, but within native's run-to-run range")
    return out


result = {"reps": reps}
if only in (None, "sso"):
    text = "".join(head) + "".join(body * 100)

    def run_sso(reader, stats):
        sink = Sink()
        singlesample.sso_genotype(os.path.join(data, "NA12878.target_loci.sorted.bam"), io.StringIO(text), sink, 20, 1, 1, 1000000,
                                  os.path.join(data, "NA12878.bam.json"), False, None, False, 1000, 1e10, None, 1000, stats=stats, **route_kw(reader))
        return "".join(l for l in sink.getvalue().splitlines(True) if not l.startswith("##fileDate"))
    result["driver_sso"] = measure(run_sso, 21100)
if only in (None, "classic"):
    with tempfile.TemporaryDirectory() as tmp:
        paths, info, sites = [], {}, None
        for k in range(8):
            path = os.path.join(tmp, "s%d.bam" % k)
            inf, sites, _ = bench._wgs_like_bam(path, genome=300_000, seed=40 + k, sample="smp%d" % k)
            info.update(inf)
            paths.append(path)
        libs = os.path.join(tmp, "libs.json")
        json.dump(info, open(libs, "w"))
        vlines = ["1\t%d\t%s\tN\t<DEL>\t0\t.\tSVTYPE=DEL;SVLEN=-%d;END=%d;STR=+-:8;CIPOS=-10,10;CIEND=-10,10;SU=8;PE=6;SR=2\n"
                  % (bp["A"]["pos"], bp["id"], bp["var_length"], bp["A"]["pos"] + bp["var_length"]) for bp in sites]
        n_rep = -(-10_500 // len(vlines))
        vtext = "".join(l for l in head if l.startswith("##")) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(vlines * n_rep)

        def run_classic(reader, stats):
            sink = Sink()
            classic.sv_genotype(",".join(paths), io.StringIO(vtext), sink, 20, 1, 1, 1000000, libs, False, None, None, False, None, 1e10,
                                stats=stats, **route_kw(reader))
            return "".join(l for l in sink.getvalue().splitlines(True) if not l.startswith("##fileDate"))
        result["driver_classic_8bam"] = measure(run_classic, 8 * len(vlines) * n_rep)
print(json.dumps(result, indent=1))

#!/usr/bin/env python
"""A/B of `svtyper -w` through reader="python" and through reader="device" (the evidence dump built on the GPU:
svt_dump_kernel.h) in ONE process on the same input, interleaved (a, b, a, b, ...): the fixture's 212 variant lines x --times
(default 20) against the fixture's BAM, the HIP engine on both sides.  Per route: wall time (median and range over --reps runs,
default 5, after one untimed run each), units per second, the size of the BAM it wrote; for the device route the counters of the
dump summed over the run's calls.  The two BAMs' inflated payloads are compared once, on the untimed runs.  Prints one JSON
object and, with --out FILE, writes it there.  GPU box only."""
import io
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svtyper_amd import classic  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, out_path = arg("--reps", 5), arg("--times", 20), arg("--out", "")
data = os.path.join(ROOT, "tests", "data")
lines = open(os.path.join(data, "example.vcf")).readlines()
text = "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * times)
n_units = 211 * times
ROUTES = ("python", "device")


class Sink(io.StringIO):
    def close(self):
        pass


def payload(path):
    """the inflated bytes of a BGZF file"""
    raw, out, at = open(path, "rb").read(), [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append(zlib.decompress(raw[at + 18:at + size - 8], -15))
        at += size
    return b"".join(out)


def run(route, out_bam, stats):
    sink = Sink()
    classic.sv_genotype(os.path.join(data, "NA12878.target_loci.sorted.bam"), io.StringIO(text), sink, 20, 1, 1, 1000000,
                        os.path.join(data, "NA12878.bam.json"), False, out_bam, None, False, None, 1e10, reader=route, stats=stats)
    return "".join(l for l in sink.getvalue().splitlines(True) if not l.startswith("##fileDate"))


result = {"reps": reps, "times": times, "n_units": n_units}
with tempfile.TemporaryDirectory() as tmp:
    bams = {r: os.path.join(tmp, r + ".bam") for r in ROUTES}
    vcfs = {r: run(r, bams[r], {}) for r in ROUTES}                  # untimed: first touch of the files, kernels loaded
    result["same_vcf"] = vcfs["python"] == vcfs["device"]
    result["same_bam_payload"] = payload(bams["python"]) == payload(bams["device"])
    result["bam_bytes"] = {r: os.path.getsize(bams[r]) for r in ROUTES}
    walls = {r: [] for r in ROUTES}
    dumps = []
    for _ in range(reps):
        for r in ROUTES:
            stats = {}
            t0 = time.perf_counter()
            run(r, bams[r], stats)
            walls[r].append((time.perf_counter() - t0) * 1e3)
            if r == "device":
                dumps.append(stats["device_reader"]["dump"])
for r in ROUTES:
    w = sorted(walls[r])
    result[r] = {"wall_ms_median": statistics.median(w), "wall_ms_min": w[0], "wall_ms_max": w[-1],
                 "units_per_s_median": n_units / statistics.median(w) * 1e3}
result["device_dump"] = {k: (statistics.median(d[k] for d in dumps) * 1e3 if k.endswith("_s") else dumps[-1][k]) for k in dumps[-1]}
result["device_dump"]["dump_ms_median"] = result["device_dump"].pop("dump_s")
result["python_over_device_wall"] = result["python"]["wall_ms_median"] / result["device"]["wall_ms_median"]
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

#!/usr/bin/env python
"""What verify="crc32" costs, in ONE process on the same inputs, routes interleaved (a-off, a-on, b-off, b-on, a-off, ...):
  scan_device_inflate   svt_bam_scan_libraries_device, compressed members uploaded, svt_inflate_kernel (+ svt_crc32_kernel)
  scan_host_inflate     svt_bam_scan_libraries_device, members inflated (+ CRC32 by libdeflate / zlib) on host threads
on the 30x whole-genome-like synthetic BAM tools/library_scan_ab.py builds (bench._wgs_like_bam, -n 1 000 000), and
  sso_device            singlesample.sso_genotype(reader="device", inflate="device")
  sso_native            singlesample.sso_genotype(reader="native")
over the fixture BAM and tests/data/example.vcf's variant lines x --lines-x (default 20).  Per route and verify setting: wall time
(median and range over --reps runs after one untimed run each), svt_bgzf_verify_stats of the last run, and on / off.  Writes
one JSON object to --out (default profiles/verify_ab.json) and prints it.  GPU box only."""
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
from svtyper_amd import native_reads, singlesample  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps = int(arg("--reps", 5))
pairs = int(arg("--pairs", 1_020_000))
lines_x = int(arg("--lines-x", 20))
out_path = arg("--out", os.path.join(ROOT, "profiles", "verify_ab.json"))
NUM_SAMP = 1_000_000
DATA = os.path.join(ROOT, "tests", "data")
FIXTURE, VCF, LIB_JSON = (os.path.join(DATA, n) for n in ("NA12878.target_loci.sorted.bam", "example.vcf", "NA12878.bam.json"))


def interleaved(legs):
    """legs: {name: fn(verify) -> stats}; every leg with verify off and on, one untimed run each, then `reps` rounds"""
    for name, fn in legs.items():
        for on in (False, True):
            fn(on)
    walls = {(n, on): [] for n in legs for on in (False, True)}
    last = {}
    for _ in range(reps):
        for name, fn in legs.items():
            for on in (False, True):
                t0 = time.perf_counter()
                last[(name, on)] = fn(on)
                walls[(name, on)].append(time.perf_counter() - t0)
    out = {}
    for name in legs:
        leg = {}
        for on in (False, True):
            w = walls[(name, on)]
            leg["on" if on else "off"] = {"wall_s_median": statistics.median(w), "wall_s_min": min(w), "wall_s_max": max(w), "stats": last[(name, on)]}
        leg["on_over_off"] = leg["on"]["wall_s_median"] / leg["off"]["wall_s_median"]
        out[name] = leg
    return out


def scan_legs(path):
    bam = native_reads.NativeBam(path)
    groups = [[rg["ID"] for rg in bam.header["RG"]]]

    def scan(inflate, on):
        bam.verify = on
        bam.scan_libraries(groups, NUM_SAMP, route="device", inflate=inflate)
        st = dict(bam.library_scan_stats)
        return {"verify": native_reads.verify_stats(), "inflate_s": st["inflate_s"], "upload_s": st["upload_s"], "members_inflated": st["members_inflated"],
                "inflated_bytes": st["inflated_bytes"], "host_reason": st["host_reason"]}

    return {"scan_device_inflate": lambda on: scan("device", on), "scan_host_inflate": lambda on: scan("host", on)}


def sso_legs():
    text = open(VCF).read().split("\n")
    head = [l for l in text if l.startswith("#")]
    body = [l for l in text if l and not l.startswith("#")]
    vcf_text = "\n".join(head + body * lines_x) + "\n"

    def sso(on, **kw):
        stats = {}
        sink = io.StringIO()
        singlesample.sso_genotype(FIXTURE, io.StringIO(vcf_text), sink, 20, 1, 1, NUM_SAMP, LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                  stats=stats, verify="crc32" if on else "off", **kw)
        return {"verify": stats["verify"], "vcf_bytes": len(sink.getvalue())}

    return {"sso_device": lambda on: sso(on, reader="device", inflate="device"), "sso_native": lambda on: sso(on, reader="native")}


result = {"reps": reps, "lines_x": lines_x, "stamp": bench.library_stamp(), "cpu": bench.cpu_model()}
if "--rocprof-leg" not in sys.argv:
    result.update(interleaved(sso_legs()))
    print(json.dumps({k: result[k] for k in ("sso_device", "sso_native")}), flush=True)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "wgs.bam")
    t0 = time.perf_counter()
    _, _, n_records = bench._wgs_like_bam(path, genome=pairs * 10, seed=7)
    print("built %s: %d records in %.0f s" % (path, n_records, time.perf_counter() - t0), flush=True)
    result["wgs_like_30x"] = {"records": n_records, "bam_bytes": os.path.getsize(path)}
    if "--rocprof-leg" in sys.argv:                         # one verified device-inflate scan and nothing else: for a kernel trace
        scan_legs(path)["scan_device_inflate"](True)
        sys.exit(0)
    result.update(interleaved(scan_legs(path)))
with open(out_path, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print(json.dumps(result, indent=1, sort_keys=True))

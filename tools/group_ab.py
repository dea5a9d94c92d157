#!/usr/bin/env python
"""What svtyper_amd.group_multiline costs per engine, in ONE process, interleaved: group_multiline.group_multiline(...) into an
in-memory sink from a file in memory (io.BytesIO: the body work, not the file system), at two sizes built from the fixture's
genotyped VCF (tests/data/example.gt.vcf, 212 single-sample lines of ~300 bytes):
  x100     its body x 100 (IDs made unique), a fifth of the lines turned into BND pairs whose mates lie half the file apart
  x5000    that x 50                                                                                (--shapes x100,x5000)
Legs:
  python   a plain-Python restatement of the loop of the reference's scripts/vcf_group_multiline.py that this tool carries as its
           checker (one timed run: it is the slow leg); its text is what the other legs must give
  host     engine="host"
  device   engine="device": the wall time, and from the call's own figures (svt_vcf_group_last_times) every step: the line table's
           kernels, the scan kernel, the compaction (two scans' worth and the key kernel), the radix passes, the match kernel and
           the plan kernels by HIP events, the upload and the download on the host's clock
`kernels`: the bytes of the body over the scan kernel's time and over all the join's kernels together, beside a device-to-device
copy of 256 MiB on the same box in the same run (torch, HIP events).  --reps timed runs (default 5) after one untimed run each,
medians with their ranges.  Prints one JSON object and, with --out FILE, writes it there.  GPU box only (--legs python,host runs
anywhere)."""
import io
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svtyper_amd import cohort, group_multiline  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, device = arg("--reps", 5), arg("--out", ""), arg("--device", 0)
SHAPES = {"x100": 100, "x5000": 5000}
shapes = arg("--shapes", "x100,x5000").split(",")
LEGS = arg("--legs", "python,host,device").split(",")
FILE_DATE = "20200229"
KERNELS = ("scan_kernel_s", "compact_kernels_s", "sort_kernels_s", "match_kernel_s", "plan_kernels_s")


def input_of(times):
    with open(os.path.join(ROOT, "tests", "data", "example.gt.vcf")) as f:
        lines = f.readlines()
    header = [l for l in lines if l.startswith("#")]
    fixture = [l.rstrip("\n").split("\t") for l in lines if not l.startswith("#")]
    body = []
    for r in range(times):
        for v in fixture:
            body.append(v[:2] + ["%s_%d" % (v[2], r)] + v[3:])
    half = len(body) // 2
    for i in range(0, half, 5):                     # lines i and i + half become mates: a fifth of the lines, half the file apart
        for k, mate in ((i, i + half), (i + half, i)):
            v = body[k]
            items = [item for item in v[7].split(";") if not item.startswith(("SVTYPE=", "MATEID="))]
            v[4], v[7] = "N[1:%d[" % (k + 1), ";".join(["SVTYPE=BND", "MATEID=" + body[mate][2]] + items)
    return ("".join(header) + "".join("\t".join(v) + "\n" for v in body)).encode()


# ------------------------------------------------------------------------------------------ the checker
def restated(vcf):
    """the script's loop over the text: its output"""
    lines = vcf.decode().split("\n")[:-1]
    header = [l + "\n" for l in lines if l.startswith("#")]
    file_format, reference, infos, alts, formats, samples = group_multiline.header_tables(header)
    out = ["\n".join(["##fileformat=" + file_format, "##fileDate=" + FILE_DATE, "##reference=" + reference] + cohort.declared_lines(infos, alts, formats)
                     + ["\t".join(header[-1].rstrip().split("\t")[:9] + samples)]) + "\n"]
    order = [f[0] for f in formats]

    def variant(text):
        v = text.rstrip().split("\t")
        keys = v[8].split(":")
        info = {}
        for item in v[7].split(";"):
            parts = item.split("=")
            info[parts[0]] = parts[1] if len(parts) > 1 else True
        return dict(v=v, keys=keys, info=info, qual=0 if v[5] == "." else float(v[5]),
                    genotypes=[dict(zip(keys, column.split(":"))) for column in v[9:9 + len(samples)]])

    def written(var, source):
        v, active = var["v"], [k for k in order if k in source["keys"]]
        return "\t".join([v[0], str(int(v[1])), v[2], v[3], v[4], "%0.2f" % source["qual"], v[6],
                          ";".join(i if t == "Flag" else "%s=%s" % (i, var["info"][i]) for i, _, t, _ in infos if i in var["info"]), ":".join(active),
                          "\t".join(":".join(g.get(k, ".") for k in active) for g in source["genotypes"])]) + "\n"

    stored = {}
    for text in lines[len(header):]:
        var = variant(text)
        if var["info"]["SVTYPE"] == "BND":
            if var["info"]["MATEID"] in stored:
                first = stored[var["info"]["MATEID"]]
                for one in (first, var):
                    [int(ci) for ci in one["info"]["CIPOS"].split(",")]
                out += [written(first, first), written(var, first)]
            else:
                stored[var["v"][2]] = var
            continue
        int(var["info"]["END"])
        for key in ("CIPOS", "CIEND"):
            [int(ci) for ci in var["info"][key].split(",")]
        out.append(written(var, var))
    return "".join(out)


# ------------------------------------------------------------------------------------------ the legs
def run(vcf, engine):
    sink, stats = io.StringIO(), {}
    t0 = time.perf_counter()
    group_multiline.group_multiline(io.BytesIO(vcf), vcf_out=sink, engine=engine, device=device, file_date=FILE_DATE, stats=stats)
    wall = time.perf_counter() - t0
    return wall, sink.getvalue(), stats


def spread(values):
    return {"ms_median": statistics.median(values) * 1e3, "ms_min": min(values) * 1e3, "ms_max": max(values) * 1e3}


def device_copy_rate():
    import torch
    n = 256 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device="cuda:%d" % device), torch.empty(n, dtype=torch.uint8, device="cuda:%d" % device)
    rates = []
    for k in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if k:
            rates.append(2 * n / (e0.elapsed_time(e1) * 1e-3))
    return statistics.median(rates)


def main():
    report = {"reps": reps, "device": device, "box": socket.gethostname(), "legs": LEGS}
    if "device" in LEGS:
        report["device_copy_bytes_per_s"] = device_copy_rate()
    for shape in shapes:
        vcf = input_of(SHAPES[shape])
        body_bytes = sum(len(l) + 1 for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#"))
        r = {"times": SHAPES[shape], "input_bytes": len(vcf), "body_bytes": body_bytes}
        want = None
        if "python" in LEGS:
            t0 = time.perf_counter()
            want = restated(vcf)
            r["python"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
        walls = {e: [] for e in ("host", "device") if e in LEGS}
        figures = []
        for rep in range(reps + 1):
            for engine in walls:                    # interleaved
                wall, text, stats = run(vcf, engine)
                if rep == 0:
                    want = want if want is not None else text
                    r.setdefault("same_text_on_every_leg", True)
                    r["same_text_on_every_leg"] &= text == want
                    r["body_lines"], r["written_lines"], r["host_lines"], r["output_bytes"] = stats["lines"], stats["written"], stats["host_lines"], len(text)
                    r["bnd_lines"] = int((stats["records"]["flags"] & 1).sum())
                    r.setdefault("host_join", {})[engine] = stats["host_join"]
                    continue
                walls[engine].append(wall)
                if engine == "device":
                    figures.append(stats["times"])
        for engine, values in walls.items():
            r[engine] = spread(values)
        if figures:
            r["device"]["per_call_ms"] = {k: {"median": statistics.median(f[k] for f in figures) * 1e3, "min": min(f[k] for f in figures) * 1e3,
                                              "max": max(f[k] for f in figures) * 1e3} for k in figures[0]}
            r["device_over_host"] = r["device"]["ms_median"] / r["host"]["ms_median"] if "host" in walls else None
            r["ranges_apart"] = ("host" in walls) and (r["device"]["ms_max"] < r["host"]["ms_min"] or r["host"]["ms_max"] < r["device"]["ms_min"])
            scan = statistics.median(f["scan_kernel_s"] for f in figures)
            join = statistics.median(sum(f[k] for k in KERNELS) for f in figures)
            r["kernels"] = {"scan_ms_median": scan * 1e3, "all_ms_median": join * 1e3, "scan_body_bytes_per_s": body_bytes / scan,
                            "all_body_bytes_per_s": body_bytes / join,
                            "scan_share_of_device_copy": body_bytes / scan / report["device_copy_bytes_per_s"],
                            "all_share_of_device_copy": body_bytes / join / report["device_copy_bytes_per_s"]}
        report[shape] = r
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What svtyper_amd.update_info costs per engine, in ONE process, interleaved: update_info.update_info(...) into an in-memory sink,
the cohort in memory (io.BytesIO: the body work, not the file system), at the two shapes of tools/classify_ab.py, built in code by
tests/updateinfocases.py:
  n100     2 120 lines x 100 samples, every line inside the rule's envelope (every line does work here)
  n1000    2 120 lines x 1 000 samples                                                             (--shapes n100,n1000)
Legs:
  python   a plain-Python restatement of the loops of the reference's scripts/update_info.py that this tool carries as its
           checker (one timed run: it is the slow leg); its text is what the other legs must give
  host     engine="host"
  device   engine="device": the wall time, and from the calls' own figures (svt_vcf_update_info_last_times, summed over the
           blocks) the line table's kernels and the update_info kernel by HIP events, the upload and the download on the host's clock
`kernel`: the bytes of the lines (each once: the head and the sample columns come from HBM once, the second look at a column
hits the cache) over the kernel's time, and the bytes it loads (the sample columns twice), beside a device-to-device copy of
256 MiB on the same box (torch, HIP events).  --reps timed runs (default 5) after one untimed run each, medians with their
ranges.  --device-block-bytes N: the device leg in blocks of N bytes of text (default: cohort.BLOCK_BYTES).  Prints one JSON
object and, with --out FILE, writes it there.  GPU box only (--legs python,host runs anywhere)."""
import io
import json
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import updateinfocases as K  # noqa: E402
from svtyper_amd import cohort, update_info  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, device = arg("--reps", 5), arg("--out", ""), arg("--device", 0)
DEVICE_BLOCK = arg("--device-block-bytes", 0)        # 0: cohort.BLOCK_BYTES["device"]
SHAPES = {"n100": 100, "n1000": 1000}
shapes = arg("--shapes", "n100,n1000").split(",")
LEGS = arg("--legs", "python,host,device").split(",")
LINES = arg("--lines", 2120)
FILE_DATE = "20200229"


def cohort_of(n):
    return (K.header(n) + "".join(K.line(1000 + 40 * k, "v%d" % k, K.cohort(n, k % 13, coarse=k % 5 > 0)) for k in range(LINES))).encode()


# ------------------------------------------------------------------------------------------ the checker
def restated(vcf):
    """the script's loops over the cohort's text: its output"""
    lines = vcf.decode().split("\n")[:-1]
    header = [l + "\n" for l in lines if l.startswith("#")]
    file_format, reference, infos, alts, formats, samples = update_info.header_tables(header)
    out = ["\n".join(["##fileformat=" + file_format, "##fileDate=" + FILE_DATE, "##reference=" + reference] + cohort.declared_lines(infos, alts, formats)
                     + ["\t".join(header[-1].rstrip().split("\t")[:9] + samples)]) + "\n"]
    order = [f[0] for f in formats]
    for text in lines[len(header):]:
        v = text.rstrip().split("\t")
        keys = v[8].split(":")
        genotypes = [dict(zip(keys, column.split(":"))) for column in v[9:9 + len(samples)]]
        info = {}
        for item in v[7].split(";"):
            parts = item.split("=")
            info[parts[0]] = parts[1] if len(parts) > 1 else True
        pe = sr = num_pos = 0
        sum_sq = 0.0
        for g in genotypes:
            pe += int(g["AP"])
            sr += int(g["AS"])
            if g["GT"] != "0/0" and g["GT"] != "./.":
                num_pos += 1
                sum_sq += float(g["SQ"])
        info.update(PE=str(pe), SR=str(sr), SU=str(pe + sr), MSQ="%0.2f" % (sum_sq / num_pos) if num_pos else ".")
        active = [k for k in order if k in keys]
        out.append("\t".join([v[0], str(int(v[1])), v[2], v[3], v[4], "%0.2f" % (0 if v[5] == "." else float(v[5])), v[6],
                              ";".join(i if t == "Flag" else "%s=%s" % (i, info[i]) for i, _, t, _ in infos if i in info), ":".join(active),
                              "\t".join(":".join(g.get(k, ".") for k in active) for g in genotypes)]) + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------ the legs
def run(vcf, engine):
    sink, stats = io.StringIO(), {}
    t0 = time.perf_counter()
    update_info.update_info(io.BytesIO(vcf), vcf_out=sink, engine=engine, device=device, file_date=FILE_DATE, stats=stats,
                            block_bytes=DEVICE_BLOCK if engine == "device" and DEVICE_BLOCK else None)
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
    report = {"reps": reps, "lines": LINES, "device": device, "box": socket.gethostname(), "legs": LEGS,
              "block_bytes": dict(cohort.BLOCK_BYTES, **({"device": DEVICE_BLOCK} if DEVICE_BLOCK else {}))}
    if "device" in LEGS:
        report["device_copy_bytes_per_s"] = device_copy_rate()
    for shape in shapes:
        vcf = cohort_of(SHAPES[shape])
        body = [l for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")]
        r = {"samples": SHAPES[shape], "input_bytes": len(vcf)}
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
                    records = np.concatenate(stats["results"])
                    r["body_lines"], r["host_lines"], r["output_bytes"] = stats["lines"], stats["host_lines"], len(text)
                    r["positive_samples"] = int(records["num_pos"].sum())
                    r.setdefault("blocks", {})[engine] = stats["blocks"]
                    continue
                walls[engine].append(wall)
                if engine == "device":
                    figures.append(stats["times"])
        for engine, values in walls.items():
            r[engine] = spread(values)
        if figures:
            r["device"]["per_call_sums_ms"] = {k: {"median": statistics.median(f[k] for f in figures) * 1e3, "min": min(f[k] for f in figures) * 1e3,
                                                   "max": max(f[k] for f in figures) * 1e3} for k in figures[0]}
            r["device_over_host"] = r["device"]["ms_median"] / r["host"]["ms_median"] if "host" in walls else None
            r["ranges_apart"] = ("host" in walls) and (r["device"]["ms_max"] < r["host"]["ms_min"] or r["host"]["ms_max"] < r["device"]["ms_min"])
            line_bytes = sum(len(l) + 1 for l in body)
            loaded = sum(len(l) + 1 + len(l.split(b"\t", 9)[-1]) for l in body)
            times = [f["update_info_kernel_s"] for f in figures]
            t = statistics.median(times)
            r["kernel"] = {"line_bytes": line_bytes, "bytes_loaded": loaded, "ms_median": t * 1e3, "ms_min": min(times) * 1e3, "ms_max": max(times) * 1e3,
                           "line_bytes_per_s": line_bytes / t, "loaded_bytes_per_s": loaded / t,
                           "share_of_device_copy": line_bytes / t / report["device_copy_bytes_per_s"]}
        report[shape] = r
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

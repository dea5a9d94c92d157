#!/usr/bin/env python
"""What decoding a BCF costs on each route, in ONE process, interleaved: an inflated BCF stream in memory to VCF text in memory by
  yardstick   tests/bcftext.py over tests/bcfreader.py, plain Python
  host        svt_bcf_text_host, the host twin of the record rule
  device      svt_bcf_text_device (one wavefront per record, lanes over samples): the whole call, and from HIP events its two
              kernels, its uploads and its download (native_reads.bcf_text_last_times)
-- medians of --reps timed runs (default 5) with their ranges, after one untimed run each; the yardstick runs --yardstick-reps
times (default: --reps; the cohort shape once, it takes a minute).  Shapes:
  single   the header of the fixture's genotyped VCF (tests/data/example.gt.vcf) and its body x 100: 21 342 lines of one sample;
  joint    the three-sample golden text (tests/golden/three.gt.vcf.gz) with its sample columns repeated to 130, its body x 20;
  cohort   the same with 1 000 samples, its body repeated to 2 120 lines.
The device's kernel bytes (the stream read once per kernel, the text written once) over the kernels' time, as a share of a
device-to-device copy on the same box (hipMemcpyDtoD of 256 MiB through torch, bytes read plus bytes written, median of --reps).
Every device text is compared with the host text on the untimed run.  Prints one JSON object and, with --out FILE, writes it
there.  GPU box only (--legs yardstick,host runs anywhere)."""
import gzip
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bcfreader as R  # noqa: E402
import bcftext as T  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, device = arg("--reps", 5), arg("--out", ""), arg("--device", 0)
yard_reps = arg("--yardstick-reps", reps)
LEGS = tuple(arg("--legs", "yardstick,host,device").split(","))
SHAPES = tuple(arg("--shapes", "single,joint,cohort").split(","))


def fixture_text():
    lines = open(os.path.join(ROOT, "tests", "data", "example.gt.vcf")).readlines()
    return "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * 100)


def joint_text(n_samples, n_lines):
    """the golden three-sample text widened to `n_samples` columns, its body repeated up to `n_lines` lines in all"""
    lines = gzip.open(os.path.join(ROOT, "tests", "golden", "three.gt.vcf.gz"), "rt").readlines()
    out, body = [], []
    for l in lines:
        cols = l.rstrip("\n").split("\t")
        if l.startswith("##"):
            out.append(l)
            continue
        wide = [cols[9 + k % 3] + ("_%d" % (k // 3) if l.startswith("#") else "") for k in range(n_samples)]
        (out if l.startswith("#") else body).append("\t".join(cols[:9] + wide) + "\n")
    return "".join(out) + "".join((body * (n_lines // len(body) + 1))[:n_lines - len(out)])


def spread(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "runs": len(ms)}


def copy_rate():
    """bytes read plus bytes written per second of a device-to-device copy of 256 MiB"""
    import torch
    n = 256 << 20
    a, b = torch.zeros(n, dtype=torch.uint8, device="cuda:%d" % device), torch.empty(n, dtype=torch.uint8, device="cuda:%d" % device)
    b.copy_(a)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return 2 * n / (statistics.median(ms) * 1e-3)


result = {"reps": reps, "device": device, "legs": list(LEGS)}
if "device" in LEGS:
    result["d2d_copy_bytes_per_s"] = copy_rate()
texts = {"single": fixture_text, "joint": lambda: joint_text(130, 241), "cohort": lambda: joint_text(1000, 2120)}
for name in SHAPES:
    text = texts[name]()
    made = nr.bcf_encode(text.encode())
    assert made["bad_line"] == 0, made
    stream = made["bytes"].tobytes()
    host = nr.bcf_text(stream)
    entry = {"stream_bytes": len(stream), "text_bytes": int(host["text_len"]), "lines": text.count("\n"), "records": int(host["n_records"]),
             "samples": int(host["n_sample"])}
    if "device" in LEGS:
        got = nr.bcf_text(stream, device=device)
        entry["device_equals_host"] = got["text"].tobytes() == host["text"].tobytes() and list(got["offsets"]) == list(host["offsets"])
        entry["host_lines"] = got["host_lines"]
    walls = {leg: [] for leg in LEGS}
    parts = []
    for rep in range(reps):
        for leg in LEGS:
            if leg == "yardstick" and rep >= (1 if name == "cohort" and "--yardstick-reps" not in sys.argv else yard_reps):
                continue
            t0 = time.perf_counter()
            if leg == "yardstick":
                T.text(stream, R)
            elif leg == "host":
                nr.bcf_text(stream)
            else:
                nr.bcf_text(stream, device=device)
            walls[leg].append((time.perf_counter() - t0) * 1e3)
            if leg == "device":
                parts.append(nr.bcf_text_last_times())
    for leg in LEGS:
        entry[leg] = spread(walls[leg])
    if parts:
        for key in parts[0]:
            entry["device"][key[:-2] + "_ms"] = spread([p[key] * 1e3 for p in parts])
        kernel_s = statistics.median(p["measure_kernel_s"] + p["write_kernel_s"] for p in parts)
        entry["device"]["kernel_bytes"] = 2 * (len(stream) - int(made["header_len"])) + int(host["text_len"] - host["header_len"])
        entry["device"]["kernel_bytes_per_s"] = entry["device"]["kernel_bytes"] / kernel_s
        entry["device"]["share_of_d2d_copy"] = entry["device"]["kernel_bytes_per_s"] / result["d2d_copy_bytes_per_s"]
    if "host" in LEGS and "device" in LEGS:
        entry["device_over_host"] = entry["device"]["ms_median"] / entry["host"]["ms_median"]
        entry["ranges_apart"] = entry["device"]["ms_max"] < entry["host"]["ms_min"] or entry["host"]["ms_max"] < entry["device"]["ms_min"]
    result[name] = entry
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

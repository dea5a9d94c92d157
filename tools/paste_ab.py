#!/usr/bin/env python
"""What the paste costs per engine, in ONE process, interleaved: svtyper_amd.paste.paste(..., afreq=True, sum_quals=True) into an
in-memory sink, inputs in memory (io.BytesIO: the body work, not the file system), at two shapes made by renaming the sample of
the fixture's genotyped VCF (tests/data/example.gt.vcf):
  n100     100 inputs x (the fixture's body x 10)
  n1000    1 000 inputs x (the fixture's body x 10)           (--shapes n100,n1000)
Legs:
  python   a plain-Python restatement of the loops of the reference's scripts/vcf_paste.py and scripts/vcf_allele_freq.py that
           this tool carries as its checker (one timed run: it is the slow leg); its text is what the other legs must give
  host     engine="host"
  device   engine="device": the wall time, and from the calls' own figures (svt_vcf_paste_last_times, summed over the blocks) the
           kernels by HIP events, the upload and the downloads on the host's clock; then once per copy layout of the write kernel
           (lane, quarter, wave), the write kernel's time alone
`write_kernel`: the bytes the write kernel reads and writes (every output byte once each way, the 12-byte place of every part,
the line records) over its time, beside a device-to-device copy of 256 MiB on the same box (torch, HIP events) and the float4
copy rate of the microarchitecture notes (6.29 TB/s).  --block-bytes: paste()'s block_bytes (default: each engine's own).  --reps timed
runs (default 3) after one untimed run each, medians.
Prints one JSON object and, with --out FILE, writes it there.  GPU box only (--legs python,host runs anywhere)."""
import io
import json
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from svtyper_amd import cohort, paste  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, device = arg("--reps", 3), arg("--out", ""), arg("--device", 0)
SHAPES = {"n100": 100, "n1000": 1000}
shapes = arg("--shapes", "n100,n1000").split(",")
LEGS = arg("--legs", "python,host,device").split(",")
TIMES = arg("--times", 10)
BLOCK_BYTES = arg("--block-bytes", 0) or None
FILE_DATE = "20200229"


def inputs_of(n):
    lines = open(os.path.join(ROOT, "tests", "data", "example.gt.vcf")).readlines()
    header = [l for l in lines if l.startswith("##")]
    chrom = next(l for l in lines if l.startswith("#CHROM")).rstrip("\n").split("\t")
    body = "".join([l for l in lines if not l.startswith("#")] * TIMES)
    first = "".join(header)
    return [((first if k == 0 else "##fileformat=VCFv4.1\n") + "\t".join(chrom[:9] + ["S%04d" % k]) + "\n" + body).encode() for k in range(n)]


# ------------------------------------------------------------------------------------------ the checker
def py2_str(x):
    text = "%.12g" % x
    return text if any(c in text for c in ".en") else text + ".0"


def restated(texts):
    """both scripts' loops over the inputs' texts (the first input is the master): the -q --afreq output"""
    files = [t.decode().split("\n")[:-1] for t in texts]
    header = [l for l in files[0] if l.startswith("##")]
    at = [next(k for k, l in enumerate(f) if not l.startswith("##")) for f in files]
    columns = files[0][at[0]].split("\t", 9)[:9]
    for f, k in zip(files, at):
        columns += f[k].rstrip().split("\t", 9)[9:]
    head, infos = paste.afreq_header(header, "\t".join(columns), FILE_DATE, False)
    order = [(row[1:], row[0] == "F") for row in infos.decode().split("\n")[:-1]]
    out = [head]
    for j in range(len(files[0]) - at[0] - 1):
        master = files[0][at[0] + 1 + j].rstrip().split("\t", 9)
        fields = master[:8]
        qual = float(fields[5])
        parts = []
        for f, k in zip(files, at):
            v = f[k + 1 + j].rstrip().split("\t", 9)
            if not parts:
                fields.append(v[8])
            qual += float(v[5])
            parts += v[9:]
        alts = len(fields[4].split(","))
        alleles, nonref = [0] * (alts + 1), 0
        for column in "\t".join(parts).split("\t"):
            gt = column.split(":")[0]
            if "." in gt:
                continue
            called = [int(a) for a in (gt.split("/") if "/" in gt else gt.split("|"))]
            for a in called:
                alleles[a] += 1
            nonref += sum(called) > 0
        total = float(sum(alleles))
        info = {}
        for pair in fields[7].split(";"):
            kv = pair.split("=")
            info[kv[0]] = kv[1] if len(kv) > 1 else True
        info["AF"] = ",".join("%.4g" % (a / total) for a in alleles[1:]) if total else ",".join("." * alts)
        info["NSAMP"] = nonref
        text = ";".join(key if flag else "%s=%s" % (key, info[key]) for key, flag in order if key in info)
        out.append("\t".join(fields[:1] + [str(int(fields[1]))] + fields[2:5] + ["%0.2f" % float(py2_str(qual)), fields[6], text, fields[8]]
                             + parts) + "\n")
    return "".join(out)


# ------------------------------------------------------------------------------------------ the legs
def run(texts, engine, layout="default"):
    sink, stats = io.StringIO(), {}
    t0 = time.perf_counter()
    paste.paste([io.BytesIO(t) for t in texts], master=io.BytesIO(texts[0]), sum_quals=True, afreq=True, vcf_out=sink, engine=engine, device=device,
                file_date=FILE_DATE, stats=stats, layout=layout, block_bytes=BLOCK_BYTES)
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
    report = {"reps": reps, "times": TIMES, "device": device, "box": socket.gethostname(), "legs": LEGS, "block_bytes": BLOCK_BYTES or cohort.BLOCK_BYTES}
    if "device" in LEGS:
        report["device_copy_bytes_per_s"] = device_copy_rate()
        report["microarch_float4_copy_bytes_per_s"] = 6.29e12
    for shape in shapes:
        texts = inputs_of(SHAPES[shape])
        r = {"inputs": len(texts), "input_bytes": sum(len(t) for t in texts)}
        want = None
        if "python" in LEGS:
            t0 = time.perf_counter()
            want = restated(texts)
            r["python"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
        walls = {e: [] for e in ("host", "device") if e in LEGS}
        figures = []
        for rep in range(reps + 1):
            for engine in walls:                    # interleaved
                wall, text, stats = run(texts, engine)
                if rep == 0:
                    want = want if want is not None else text
                    r.setdefault("same_text_on_every_leg", True)
                    r["same_text_on_every_leg"] &= text == want
                    r["lines"], r["host_lines"], r["output_bytes"] = stats["lines"], stats["host_lines"], len(text)
                    r.setdefault("blocks", {})[engine] = stats["blocks"]
                    continue
                walls[engine].append(wall)
                if engine == "device":
                    figures.append(stats["times"])
        for engine, values in walls.items():
            r[engine] = spread(values)
        if figures:
            r["device"]["per_call_sums_ms"] = {k: statistics.median(f[k] for f in figures) * 1e3 for k in figures[0]}
            r["device_over_host"] = r["device"]["ms_median"] / r["host"]["ms_median"] if "host" in walls else None
            cells = r["lines"] * len(texts)
            moved = 2 * r["output_bytes"] + 12 * cells + 64 * r["lines"]
            r["write_kernel"] = {"bytes_moved": moved, "layouts": {}}
            for layout in ("lane", "quarter", "wave"):
                got = []
                for rep in range(reps + 1):
                    _wall, text, stats = run(texts, "device", layout)
                    assert text == want, layout
                    if rep:
                        got.append(stats["times"]["write_kernel_s"])
                t = statistics.median(got)
                r["write_kernel"]["layouts"][layout] = {"ms_median": t * 1e3, "ms_min": min(got) * 1e3, "bytes_per_s": moved / t,
                                                        "share_of_device_copy": moved / t / report["device_copy_bytes_per_s"]}
        report[shape] = r
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

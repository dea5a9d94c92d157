#!/usr/bin/env python
"""What the classifier costs per engine, in ONE process, interleaved: svtyper_amd.classify.classify(...) into an in-memory sink, the
cohort in memory (io.BytesIO: the body work, not the file system), at two shapes built in code by tests/classifycases.py:
  n100     2 120 lines x 100 samples, every other line a DEL or DUP (both tests, both verdicts), the rest BND and INV lines
  n1000    2 120 lines x 1 000 samples                                                             (--shapes n100,n1000)
Legs:
  python   a plain-Python restatement of the loops of the reference's scripts/sv_classifier.py that this tool carries as its
           checker (numpy's median, the regression from centred sums; one timed run: it is the slow leg); its text is what the
           other legs must give
  host     engine="host"
  device   engine="device": the wall time, and from the calls' own figures (svt_vcf_classify_last_times, summed over the blocks)
           the kernel by HIP events, the upload and the download on the host's clock
`kernel`: the bytes the classify kernel reads (every byte of a DEL/DUP line once per pass over its samples: two passes on the
low-frequency route, three with carriers, two or three on the regression's; the first columns of the other lines) over its
time, beside a device-to-device copy of 256 MiB on the same box (torch, HIP events).  --reps timed runs (default 3) after one
untimed run each, medians.  Prints one JSON object and, with --out FILE, writes it there.  GPU box only (--legs python,host
runs anywhere)."""
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
import classifycases as K  # noqa: E402
from svtyper_amd import classify, cohort  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, out_path, device = arg("--reps", 3), arg("--out", ""), arg("--device", 0)
SHAPES = {"n100": 100, "n1000": 1000}
shapes = arg("--shapes", "n100,n1000").split(",")
LEGS = arg("--legs", "python,host,device").split(",")
LINES = arg("--lines", 2120)
FILE_DATE = "20200229"


def cohort_of(n):
    body = []
    for k in range(LINES // 2):
        svtype, supported = ("DEL", "DUP")[k % 2], k % 4 < 2
        n_pos = (3 + k % 7) if k % 3 else min(n - 1, 12 + k % 40)
        body.append(K.line("1", 1000 + 40 * k, "v%d" % k, svtype, K.columns(*K.cohort(n, n_pos, svtype, supported, salt=k % 11, coarse=k % 5 > 0))))
        body.append(K.other("1", 1020 + 40 * k, "o%d" % k, ("BND", "INV")[k % 2], n))
    return (K.header(n) + "".join(body)).encode(), K.genders(n).encode()


# ------------------------------------------------------------------------------------------ the checker
def regression(x, y):
    x, y = np.asarray(x), np.asarray(y)
    dx, dy = x - x.mean(), y - y.mean()
    return float((dx * dy).sum() / (dx * dx).sum()), float((dx * dy).sum() ** 2 / ((dx * dx).sum() * (dy * dy).sum()))


def restated(vcf, genders):
    """the script's loops over the cohort's text (no -e, no -a, the default thresholds): its output"""
    gender = {v[0]: int(v[1]) for v in (l.split("\t") for l in genders.decode().splitlines())}
    lines = vcf.decode().split("\n")[:-1]
    header = [l for l in lines if l.startswith("#")]
    _ff, _ref, _filters, infos, alts, formats = cohort.header_attributes([h for h in header if h.startswith("##")], ValueError)
    samples = header[-1].split("\t")[9:]
    out = ["\n".join(["##fileformat=VCFv4.2", "##fileDate=" + FILE_DATE, "##reference=ref.fa"] + cohort.declared_lines(infos, alts, formats)
                     + ["\t".join(header[-1].split("\t")[:9] + samples)]) + "\n"]
    for number, text in enumerate(lines[len(header):]):
        first = next((i.split("=")[1] for i in text.rstrip().split("\t")[7].split(";") if i.startswith("SVTYPE=")), None)
        if first not in ("DEL", "DUP"):
            out.append(text + "\n")
            continue
        var = classify._Variant(text + "\n", samples, infos, formats, "cohort", number)
        sign = -1.0 if var.info["SVTYPE"] == "DEL" else 1.0
        sex = var.first[0] in ("X", "Y")
        gts = [g["GT"] for g in var.genotypes]
        if sum(g not in ("./.", "0/0") for g in gts) < 10:
            cn = [float(g["CN"]) for g in var.genotypes]
            ref = [c for c, g in zip(cn, gts) if g == "0/0"]
            alt = [c for c, g in zip(cn, gts) if g in ("0/1", "1/1")]
            kept = False
            if ref and alt:
                median = np.median(ref)
                mad = np.median(np.abs(np.array(ref) - median))
                kept = sum(sign * (c - median) > 2 * mad and sign * (c - median) > 0.5 for c in alt) / float(len(alt)) > 0.5
        else:
            pairs = [(float(g["AB"]), float(g["CN"]) * (2 if sex and gender[s] == 1 else 1)) for s, g in zip(samples, var.genotypes) if g["AB"] != "."]
            pairs = [p for p in pairs if p[0] != -1]
            kept = False
            if len({p[0] for p in pairs}) > 1 and len({p[1] for p in pairs}) > 1:
                slope, r2 = regression([p[0] for p in pairs], [p[1] for p in pairs])
                kept = not r2 < 0.2 and not sign * slope < 1.0
        if kept:
            out.append(var.text(var.first[4]))
            continue
        ident, end, pos, chrom = var.first[2], var.info["END"], var.pos, var.first[0]
        swapped = {"CIPOS": var.info["CIEND"], "CIEND": var.info["CIPOS"], "CIPOS95": var.info["CIEND95"], "CIEND95": var.info["CIPOS95"]}
        base = {k: v for k, v in var.info.items() if k not in ("SVLEN", "END")}
        for mate in (1, 2):
            var.info = dict(base, SVTYPE="BND", EVENT=ident, MATEID="%s_%d" % (ident, 3 - mate), **(swapped if mate == 2 else {}))
            if mate == 2:
                var.info["SECONDARY"] = True
            var.first[2], var.pos = "%s_%d" % (ident, mate), pos if mate == 1 else end
            there = "%s:%s" % (chrom, end if mate == 1 else pos)
            out.append(var.text("N[%s[" % there if (sign < 0) == (mate == 1) else "]%s]N" % there))
    return "".join(out)


# ------------------------------------------------------------------------------------------ the legs
def run(vcf, genders, engine):
    sink, stats = io.StringIO(), {}
    t0 = time.perf_counter()
    classify.classify(io.BytesIO(vcf), io.BytesIO(genders), vcf_out=sink, engine=engine, device=device, file_date=FILE_DATE, stats=stats)
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


def kernel_bytes(vcf, records):
    """what the kernel reads: a line's sample columns once for the tabs, once for the samples, and once per further pass"""
    body = [l for l in vcf.split(b"\n")[:-1] if not l.startswith(b"#")]
    moved = 0
    for line, r in zip(body, records):
        if r["route"] == nr.CLASSIFY_VERBATIM:
            moved += len(line) - len(line.split(b"\t", 9)[-1])
        elif r["route"] == nr.CLASSIFY_LOW:
            moved += len(line) * (3 + (r["n_ref"] > 0))
        else:
            moved += len(line) * (3 + (r["slope"] != 0))
    return int(moved) + 64 * len(body)


def main():
    report = {"reps": reps, "lines": LINES, "device": device, "box": socket.gethostname(), "legs": LEGS, "block_bytes": cohort.BLOCK_BYTES}
    if "device" in LEGS:
        report["device_copy_bytes_per_s"] = device_copy_rate()
    for shape in shapes:
        vcf, genders = cohort_of(SHAPES[shape])
        r = {"samples": SHAPES[shape], "input_bytes": len(vcf)}
        want = None
        if "python" in LEGS:
            t0 = time.perf_counter()
            want = restated(vcf, genders)
            r["python"] = {"ms": (time.perf_counter() - t0) * 1e3, "runs": 1}
        walls = {e: [] for e in ("host", "device") if e in LEGS}
        figures, records = [], None
        for rep in range(reps + 1):
            for engine in walls:                    # interleaved
                wall, text, stats = run(vcf, genders, engine)
                if rep == 0:
                    want = want if want is not None else text
                    r.setdefault("same_text_on_every_leg", True)
                    r["same_text_on_every_leg"] &= text == want
                    records = np.concatenate(stats["results"])
                    r["body_lines"], r["host_lines"], r["near_lines"], r["output_bytes"] = stats["lines"], stats["host_lines"], stats["near_lines"], len(text)
                    r["routes"] = {name: int((records["route"] == code).sum()) for name, code in (("verbatim", 0), ("low", 1), ("high", 2))}
                    r["kept"] = int(records["verdict"].sum())
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
            moved, t = kernel_bytes(vcf, records), statistics.median(f["classify_kernel_s"] for f in figures)
            r["kernel"] = {"bytes_read": moved, "ms_median": t * 1e3, "ms_min": min(f["classify_kernel_s"] for f in figures) * 1e3,
                           "bytes_per_s": moved / t, "share_of_device_copy": moved / t / report["device_copy_bytes_per_s"]}
        report[shape] = r
    text = json.dumps(report, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""What --bcf costs and saves against --bgzf, in ONE process, interleaved: bcf_out.open_bcf and bgzf_out.open_text over an in-memory
sink, per deflate choice (zlib, host, device) in three modes --
  plain       no option
  sort        sort=True
  sort_csi    sort=True and a .csi (open_bcf: index="csi"; open_text: index="tbi", csi=True)
-- timed from the first write() to the end of close().  bgzf_out.py and everything under it are the parent commit's, byte for
byte, so the `bgzf` legs measured here, in the same session, are the parent's.  --reps timed runs (default 5) after one untimed
run each.  Inputs:
  vcf      the header of the fixture's genotyped VCF (tests/data/example.gt.vcf) and its body x 100: single-sample lines of ~300 bytes;
  joint    the three-sample golden text (tests/golden/three.gt.vcf.gz) with its sample columns repeated to 130 and its body
           x --times (default 20): the joint shape, where the individual part is the record.
For the device legs the kernels' own times from HIP events: the two record kernels (svt_bcf_last_times) beside the line-table
kernels (svt_vcf_lines_last_times) and the deflate kernels (svt_bgzf_deflate_last_times) of the same call; `host_twin`: the
record encoder alone on the host (svt_bcf_encode_host) against the same on the device (svt_bcf_encode_device, upload and download
included), so that a leg where the device encoder loses shows.  Every BCF is read back by tests/bcfreader.py on the untimed runs
and compared with the text field for field; device files are compared with host files.  Prints one JSON object and, with --out
FILE, writes it there.  GPU box only (--deflate zlib,host runs anywhere)."""
import gzip
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bcfreader as R  # noqa: E402
from svtyper_amd import bcf_out, bgzf_out  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, out_path, device = arg("--reps", 5), arg("--times", 20), arg("--out", ""), arg("--device", 0)
DEFLATES = tuple(arg("--deflate", "zlib,host,device").split(","))


def fixture_text():
    lines = open(os.path.join(ROOT, "tests", "data", "example.gt.vcf")).readlines()
    return "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * 100)


def joint_text(n_samples=130):
    lines = gzip.open(os.path.join(ROOT, "tests", "golden", "three.gt.vcf.gz"), "rt").readlines()
    out, body = [], []
    for l in lines:
        cols = l.rstrip("\n").split("\t")
        if l.startswith("##"):
            out.append(l)
            continue
        wide = [cols[9 + k % 3] + ("_%d" % (k // 3) if l.startswith("#") else "") for k in range(n_samples)]
        (out if l.startswith("#") else body).append("\t".join(cols[:9] + wide) + "\n")
    return "".join(out) + "".join(body * times)


def run(kind, text, index_path, deflate, mode):
    """(seconds from the first write() to the end of close(), the file's bytes)"""
    sink = io.BytesIO()
    kept = []
    sink.close = lambda: kept.append(sink.getvalue())
    sort, index = mode != "plain", mode == "sort_csi"
    t0 = time.perf_counter()
    if kind == "bcf":
        out = bcf_out.open_bcf(sink, deflate=deflate, device=device, sort=sort, index="csi" if index else None, index_path=index_path if index else None)
    else:
        out = bgzf_out.open_text(sink, deflate=deflate, device=device, sort=sort, index="tbi" if index else None, csi=index,
                                 index_path=index_path if index else None)
    for at in range(0, len(text), 1 << 16):                          # (in pieces, as a driver writes)
        out.write(text[at:at + (1 << 16)])
    out.close()
    return time.perf_counter() - t0, kept[0]


def stats(ms):
    return {"wall_ms_median": statistics.median(ms), "wall_ms_min": min(ms), "wall_ms_max": max(ms)}


MODES = ("plain", "sort", "sort_csi")
result = {"reps": reps, "times": times, "device": device, "deflates": list(DEFLATES)}
with tempfile.TemporaryDirectory() as tmp:
    index_path = os.path.join(tmp, "t.csi")
    for name, text in (("vcf", fixture_text()), ("joint", joint_text())):
        data = text.encode()
        entry = {"text_bytes": len(data), "lines": text.count("\n"), "samples": text[:text.index("\n", text.index("#CHROM"))].count("\t") - 8}
        legs = [(kind, deflate, mode) for deflate in DEFLATES for mode in MODES for kind in ("bgzf", "bcf")]
        files = {}
        for leg in legs:                                              # untimed: the library loaded, the kernels loaded
            _t, files[leg] = run(leg[0], text, index_path, leg[1], leg[2])
        body = [l for l in text.split("\n") if l and not l.startswith("#")]
        head, d, records, _ = R.read_bcf(R.stream_of(files["bcf", DEFLATES[0], "plain"]))
        entry["bcf_reads_back"] = head == text[:len(head)] and len(records) == len(body) and all(r == R.line_fields(l, d) for r, l in zip(records, body))
        entry["same_stream_on_every_route"] = len({R.stream_of(files["bcf", deflate, "sort"]) for deflate in DEFLATES}) == 1
        if "device" in DEFLATES and "host" in DEFLATES:
            entry["device_equals_host"] = all(files["bcf", "device", mode] == files["bcf", "host", mode] for mode in MODES)
        entry["bytes"] = {deflate: {"vcf_gz": len(files["bgzf", deflate, "plain"]), "bcf": len(files["bcf", deflate, "plain"]),
                                    "bcf_over_vcf_gz": len(files["bcf", deflate, "plain"]) / len(files["bgzf", deflate, "plain"])} for deflate in DEFLATES}
        entry["stream_bytes"] = len(R.stream_of(files["bcf", DEFLATES[0], "plain"]))
        walls = {leg: [] for leg in legs}
        kernels, twin = [], {"host_ms": [], "device_ms": []}
        for _ in range(reps):
            for leg in legs:
                t, _raw = run(leg[0], text, index_path, leg[1], leg[2])
                walls[leg].append(t * 1e3)
                if leg == ("bcf", "device", "sort_csi"):
                    kernels.append(dict(nr.bcf_last_times(), **{"lines_" + k: v for k, v in nr.vcf_lines_last_times().items()},
                                        **{"deflate_" + k: v for k, v in nr.bgzf_deflate_last_times().items()},
                                        **{"index_" + k: v for k, v in nr.bam_index_last_times().items()}))
            t0 = time.perf_counter()
            nr.bcf_encode(data)
            twin["host_ms"].append((time.perf_counter() - t0) * 1e3)
            if "device" in DEFLATES:
                t0 = time.perf_counter()
                made = nr.bcf_encode(data, device=device)
                twin["device_ms"].append((time.perf_counter() - t0) * 1e3)
                twin["host_lines"] = made["host_lines"]
        for deflate in DEFLATES:
            entry[deflate] = {mode: {kind: stats(walls[kind, deflate, mode]) for kind in ("bgzf", "bcf")} for mode in MODES}
            for mode in MODES:
                entry[deflate][mode]["bcf_over_bgzf"] = entry[deflate][mode]["bcf"]["wall_ms_median"] / entry[deflate][mode]["bgzf"]["wall_ms_median"]
        entry["encoder_alone"] = {k: (statistics.median(v) if isinstance(v, list) and v else v) for k, v in twin.items() if v != []}
        if kernels:
            entry["device"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0] if k.endswith("kernel_s")}
        result[name] = entry
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

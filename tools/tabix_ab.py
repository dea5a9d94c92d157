#!/usr/bin/env python
"""What --sort and --tabix cost at close(), in ONE process, interleaved: bgzf_out.open_text over an in-memory sink, per deflate
choice (zlib, host, device) in three modes --
  plain        no option: the writer as it was, the baseline (its wall time is write() of the whole text and close())
  index        index="tbi" over text that is sorted already
  sort_index   sort=True, index="tbi" over the text as the drivers write it
-- and `python_index`: the checker's index build in plain Python (tests/tbxcases.py: build_tbi) over the sorted text, the CPU
yardstick for the native fold.  --reps timed runs (default 5) after one untimed run each.  Inputs:
  vcf      the header of the fixture's genotyped VCF (tests/data/example.gt.vcf) and its body x 100 (tools/deflate_ab.py's main
           input, with the header once: a '#' line in the body is not indexable);
  vcf_in   the fixture's input VCF (tests/data/example.vcf), header once and body x --times (default 20): the text that
           deflate_ab's second workload reads (its own second input is BAM records, which are no VCF text).
For the device legs the kernels' own times from HIP events: the line-table and gather kernels (svt_vcf_lines_last_times) beside
the deflate kernels of the same call (svt_bgzf_deflate_last_times).  Every file is inflated and compared with the expected text
once, on the untimed runs, and device files with host files.  Prints one JSON object and, with --out FILE, writes it there.
GPU box only.

--deflate device (a comma-separated choice of zlib,host,device; default all three) times those legs alone, and --package-root
DIR takes svtyper_amd from another built checkout: how one commit is measured against another in one session
(profiles/held_close_ab.json)."""
import gzip
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[sys.argv.index("--package-root") + 1] if "--package-root" in sys.argv else ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tbxcases as X  # noqa: E402
from svtyper_amd import bgzf_out  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, out_path, device = arg("--reps", 5), arg("--times", 20), arg("--out", ""), arg("--device", 0)
DEFLATES = tuple(arg("--deflate", "zlib,host,device").split(","))
data = os.path.join(ROOT, "tests", "data")


def repeated(name, n):
    lines = open(os.path.join(data, name), "rb").readlines()
    return b"".join(l for l in lines if l.startswith(b"#")) + b"".join([l for l in lines if not l.startswith(b"#")] * n)


def close_time(text, index_path, **options):
    """(seconds from the first write() to the end of close(), the file's bytes)"""
    sink = io.BytesIO()
    kept = []
    sink.close = lambda: kept.append(sink.getvalue())
    piece = text.decode()
    t0 = time.perf_counter()
    out = bgzf_out.open_text(sink, index_path=index_path if options.get("index") else None, **options)
    for at in range(0, len(piece), 1 << 16):                         # (in pieces, as a driver writes; the text is ASCII)
        out.write(piece[at:at + (1 << 16)])
    out.close()
    return time.perf_counter() - t0, kept[0]


MODES = {"plain": {}, "index": {"index": "tbi"}, "sort_index": {"sort": True, "index": "tbi"}}
result = {"reps": reps, "times": times, "device": device, "deflates": list(DEFLATES), "package_root": arg("--package-root", ROOT)}
with tempfile.TemporaryDirectory() as tmp:
    index_path = os.path.join(tmp, "t.tbi")
    for name, text in (("vcf", repeated("example.gt.vcf", 100)), ("vcf_in", repeated("example.vcf", times))):
        ordered = X.sorted_text(text)
        entry = {"text_bytes": len(text), "lines": text.count(b"\n")}
        legs = [(deflate, mode) for deflate in DEFLATES for mode in MODES]
        files, ok = {}, True
        for deflate, mode in legs:                                     # untimed: the library loaded, the kernels loaded
            _t, files[deflate, mode] = close_time(ordered if mode == "index" else text, index_path, deflate=deflate, device=device, **MODES[mode])
            ok = ok and gzip.decompress(files[deflate, mode]) == (text if mode == "plain" else ordered)
            if mode != "plain":
                tbi = X.read_tbi(open(index_path, "rb").read())
                X.check_structure(files[deflate, mode], tbi)
        entry["round_trip_and_structure"] = ok
        if "device" in DEFLATES and "host" in DEFLATES:
            entry["device_equals_host"] = all(files["device", mode] == files["host", mode] for mode in MODES)
        walls = {leg: [] for leg in legs}
        python_index, kernels = [], []
        member_off = X.Members(files[DEFLATES[0], "index"]).order
        for _ in range(reps):
            for deflate, mode in legs:
                t, _raw = close_time(ordered if mode == "index" else text, index_path, deflate=deflate, device=device, **MODES[mode])
                walls[deflate, mode].append(t * 1e3)
                if (deflate, mode) == ("device", "sort_index"):
                    kernels.append(dict(nr.vcf_lines_last_times(), **{"deflate_" + k: v for k, v in nr.bgzf_deflate_last_times().items()}))
            t0 = time.perf_counter()
            X.build_tbi(ordered, member_off)
            python_index.append((time.perf_counter() - t0) * 1e3)
        for deflate in DEFLATES:
            entry[deflate] = {mode: {"wall_ms_median": statistics.median(walls[deflate, mode]), "wall_ms_min": min(walls[deflate, mode]),
                                     "wall_ms_max": max(walls[deflate, mode])} for mode in MODES}
            base = entry[deflate]["plain"]["wall_ms_median"]
            entry[deflate]["index_over_plain"] = entry[deflate]["index"]["wall_ms_median"] / base
            entry[deflate]["sort_index_over_plain"] = entry[deflate]["sort_index"]["wall_ms_median"] / base
        entry["python_index"] = {"wall_ms_median": statistics.median(python_index), "wall_ms_min": min(python_index)}
        if "device" not in DEFLATES:
            result[name] = entry
            continue
        entry["device"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0] if k.endswith("kernel_s")}
        lines_ms = sum(v for k, v in entry["device"]["kernels_ms_median"].items() if not k.startswith("deflate_"))
        entry["device"]["line_kernels_over_deflate_kernel"] = lines_ms / entry["device"]["kernels_ms_median"]["deflate_deflate_kernel_ms"]
        result[name] = entry
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

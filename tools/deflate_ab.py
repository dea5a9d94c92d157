#!/usr/bin/env python
"""A/B/C of BGZF deflate in ONE process, interleaved (zlib, host, device, zlib, ...): zlib at level 6 as bam.BgzfWriter runs it
(deflate="zlib"), the one-source compressor on the host (svt_bgzf_deflate_host) and on the device (svt_bgzf_deflate_device), each
over whole lists of member payloads, --reps timed runs (default 5) after one untimed run each.  Inputs:
  vcf   the fixture's genotyped VCF text (tests/data/example.gt.vcf) x 100, cut every 65 280 bytes as bgzf_out.open_text cuts it;
  bam   the members' payloads of the `-w` BAM that tools/write_alignment_ab.py's workload writes (the fixture's 212 variant lines
        x --times, default 20, reader="device"), cut as bam.AlignmentFile cut them.
Per input and method: wall time (median, min, max), bytes out, the ratio to the payload; for the device the kernels' own times
from HIP events (svt_bgzf_deflate_last_times), apart from upload and download.  All three outputs are inflated and compared
with the payload once, on the untimed runs.  Prints one JSON object and, with --out FILE, writes it there.  GPU box only.

--huffman: two more legs in the same interleaving, host_dynamic and device_dynamic (huffman="dynamic": svt_bgzf_deflate_host_mode /
_device_mode with SVT_DEFLATE_DYNAMIC), with their own kernel times, the ratios of the dynamic device leg to the fixed one, the
fixed kernel's spread over the reps, and `code_construction`: svt_huffman_lengths_device over three histograms per member (286, 30
and 19 symbols: the member's byte counts with every length symbol used, and flat ones), as whole calls on the host's clock -- an
upper bound on what the code's construction adds to the kernel, since launches and copies are in it.  Without the flag the
output is what it was."""
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
from svtyper_amd import bam, classic  # noqa: E402
from svtyper_amd.bgzf import PAYLOAD  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, out_path, device = arg("--reps", 5), arg("--times", 20), arg("--out", ""), arg("--device", 0)
huffman = "--huffman" in sys.argv
data = os.path.join(ROOT, "tests", "data")


def vcf_payloads():
    with open(os.path.join(data, "example.gt.vcf"), "rb") as f:
        text = f.read() * 100
    return [text[i:i + PAYLOAD] for i in range(0, len(text), PAYLOAD)]


def bam_payloads():
    class Sink(io.StringIO):
        def close(self):
            pass
    lines = open(os.path.join(data, "example.vcf")).readlines()
    text = "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * times)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.bam")
        classic.sv_genotype(os.path.join(data, "NA12878.target_loci.sorted.bam"), io.StringIO(text), Sink(), 20, 1, 1, 1000000,
                            os.path.join(data, "NA12878.bam.json"), False, path, None, False, None, 1e10, reader="device")
        raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append(zlib.decompress(raw[at + 18:at + size - 8], -15))
        at += size
    return out[:-1]                                                  # (without the EOF member)


def by_zlib(payloads):
    sink = io.BytesIO()
    sink.close = lambda: None
    w = bam.BgzfWriter(sink, level=6, deflate="zlib")
    for p in payloads:
        w._member(p)
    return sink.getvalue()


METHODS = {"zlib6": by_zlib,
           "host": lambda payloads: nr.bgzf_deflate(payloads)[0].tobytes(),
           "device": lambda payloads: nr.bgzf_deflate(payloads, device=device)[0].tobytes()}
if huffman:
    METHODS["host_dynamic"] = lambda payloads: nr.bgzf_deflate(payloads, huffman="dynamic")[0].tobytes()
    METHODS["device_dynamic"] = lambda payloads: nr.bgzf_deflate(payloads, device=device, huffman="dynamic")[0].tobytes()


def code_construction(payloads):
    """svt_huffman_lengths_device over stand-ins for the members' three histograms: wall time per call set, median of reps"""
    import numpy as np
    lit = np.zeros((len(payloads), 286), np.uint32)
    for k, p in enumerate(payloads):
        lit[k, :256] = np.bincount(np.frombuffer(p, np.uint8), minlength=256)
        lit[k, 256:] = 1 + np.arange(30) % 7
    dist = np.tile(1 + np.arange(30, dtype=np.uint32) * 37 % 101, (len(payloads), 1))
    cl = np.tile(1 + np.arange(19, dtype=np.uint32) * 13 % 29, (len(payloads), 1))
    walls = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        nr.huffman_lengths(lit, 15, device=device)
        nr.huffman_lengths(dist, 15, device=device)
        nr.huffman_lengths(cl, 7, device=device)
        walls.append((time.perf_counter() - t0) * 1e3)
    return {"calls": 3, "wall_ms_median": statistics.median(walls[1:]), "wall_ms_min": min(walls[1:])}


def inflate_all(raw):
    out, at = [], 0
    while at < len(raw):
        size = struct.unpack_from("<H", raw, at + 16)[0] + 1
        out.append(zlib.decompress(raw[at + 18:at + size - 8], -15))
        at += size
    return b"".join(out)


result = {"reps": reps, "times": times, "device": device}
for name, payloads in (("vcf", vcf_payloads()), ("bam", bam_payloads())):
    total = sum(len(p) for p in payloads)
    entry = {"members": len(payloads), "payload_bytes": total}
    outs = {m: fn(payloads) for m, fn in METHODS.items()}            # untimed: the library loaded, the kernels loaded
    entry["round_trip"] = all(inflate_all(o) == b"".join(payloads) for o in outs.values())
    entry["device_equals_host"] = outs["device"] == outs["host"]
    walls, kernels, kernels_dynamic = {m: [] for m in METHODS}, [], []
    for _ in range(reps):
        for m, fn in METHODS.items():
            t0 = time.perf_counter()
            fn(payloads)
            walls[m].append((time.perf_counter() - t0) * 1e3)
            if m == "device":
                kernels.append(nr.bgzf_deflate_last_times())
            if m == "device_dynamic":
                kernels_dynamic.append(nr.bgzf_deflate_last_times())
    for m in METHODS:
        w = sorted(walls[m])
        entry[m] = {"wall_ms_median": statistics.median(w), "wall_ms_min": w[0], "wall_ms_max": w[-1], "bytes_out": len(outs[m]),
                    "ratio": len(outs[m]) / total, "payload_MB_per_s_median": total / statistics.median(w) / 1e3}
    entry["device"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0]}
    entry["device_over_zlib6_wall"] = entry["device"]["wall_ms_median"] / entry["zlib6"]["wall_ms_median"]
    entry["host_over_zlib6_wall"] = entry["host"]["wall_ms_median"] / entry["zlib6"]["wall_ms_median"]
    if huffman:
        entry["host_dynamic_equals_device_dynamic"] = outs["device_dynamic"] == outs["host_dynamic"]
        entry["device_dynamic"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels_dynamic) * 1e3 for k in kernels_dynamic[0]}
        fixed_kernel = sorted(t["deflate_kernel_s"] * 1e3 for t in kernels)
        entry["device"]["deflate_kernel_ms_min_max"] = [fixed_kernel[0], fixed_kernel[-1]]
        entry["dynamic_over_fixed_deflate_kernel"] = (entry["device_dynamic"]["kernels_ms_median"]["deflate_kernel_ms"]
                                                      / entry["device"]["kernels_ms_median"]["deflate_kernel_ms"])
        entry["dynamic_over_fixed_device_wall"] = entry["device_dynamic"]["wall_ms_median"] / entry["device"]["wall_ms_median"]
        entry["device_dynamic_over_zlib6_wall"] = entry["device_dynamic"]["wall_ms_median"] / entry["zlib6"]["wall_ms_median"]
        entry["code_construction"] = code_construction(payloads)
    result[name] = entry
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

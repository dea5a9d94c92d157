#!/usr/bin/env python
"""What a CSI index costs at close(), in ONE process, the legs interleaved: bam.AlignmentFile(path, "wb", sort=True, index="bai", ...)
with --deflate device in three legs --
  bai          today's route, the baseline: the .bai folded on the host (svt_bai_build)
  csi_host     csi=True with the fold on the host (svt_csi_build_bam)
  csi_device   csi=True with the fold on the GPU behind the members (svt_bam_sorted_bgzf_csi_device)
-- and with --deflate host in two, bai and csi; from the first write_raw() to the end of close().  --reps timed runs (default 5)
after one untimed run each.  Inputs as tools/bam_sort_ab.py's: `bam`, the records of the `-w` BAM of the fixture's workload, and
`bam_x`, the same records --copies times (default 50).  Beside the walls: the new kernels' times from HIP events
(svt_bam_index_last_times) next to the deflate kernel of the same call, and the folds alone over the written file's tables --
svt_bai_build, svt_csi_build_bam and svt_bam_index_fold_device (which uploads the span table: the one-call entry does not).
Checked on the untimed runs: the BAM is the same file in every leg of a deflate choice, the device fold's .csi is the host
fold's byte for byte, and on `bam` the index answers what tests/csioutcases.py's reader asks.  Prints one JSON object and, with
--out FILE, writes it there (profiles/csi_ab.json).  GPU box only."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import baicases as B  # noqa: E402
import csioutcases as K  # noqa: E402
from svtyper_amd import bam  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


reps, times, copies, out_path, device = arg("--reps", 5), arg("--times", 20), arg("--copies", 50), arg("--out", ""), arg("--device", 0)
data = os.path.join(ROOT, "tests", "data")
IN_BAM = os.path.join(data, "NA12878.target_loci.sorted.bam")


def dump():
    """(the template, the records) of the `-w` BAM of tools/deflate_ab.py's workload (tools/bam_sort_ab.py's dump)"""
    import io

    from svtyper_amd import classic

    class Sink(io.StringIO):
        def close(self):
            pass
    lines = open(os.path.join(data, "example.vcf")).readlines()
    text = "".join(l for l in lines if l.startswith("#")) + "".join([l for l in lines if not l.startswith("#")] * times)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "w.bam")
        classic.sv_genotype(IN_BAM, io.StringIO(text), Sink(), 20, 1, 1, 1000000, os.path.join(data, "NA12878.bam.json"), False, path, None,
                            False, None, 1e10, reader="device")
        w = B.Written(open(path, "rb").read())
    return bam.AlignmentFile(IN_BAM, "rb"), w.records


def moved(records, k):
    import struct
    out = []
    for raw in records:
        tid, pos = struct.unpack_from("<ii", raw, 4)
        out.append(raw if tid < 0 or k == 0 else raw[:8] + struct.pack("<i", pos + 37 * k) + raw[12:])
    return out


LEGS = {("device", "bai"): dict(), ("device", "csi_host"): dict(csi=True), ("device", "csi_device"): dict(csi=True),
        ("host", "bai"): dict(), ("host", "csi"): dict(csi=True)}


def close_time(path, template, records, deflate, leg):
    t0 = time.perf_counter()
    out = bam.AlignmentFile(path, "wb", template=template, device=device, deflate=deflate, sort=True, index="bai", **LEGS[deflate, leg])
    out._device_fold = leg == "csi_device"
    for raw in records:
        out.write_raw(raw)
    out.close()
    return time.perf_counter() - t0


def median_ms(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


result = {"reps": reps, "times": times, "copies": copies, "device": device}
template, fixture = dump()
n_ref, l_ref_max = len(template.references), max(template.lengths)
result["depth"] = nr.csi_depth(l_ref_max)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "ev.bam")
    for name, records in (("bam", fixture), ("bam_x", [raw for k in range(copies) for raw in moved(fixture, k)])):
        entry = {"records": len(records), "record_bytes": sum(len(r) for r in records)}
        files = {}
        for deflate, leg in LEGS:                                       # untimed: the library loaded, the kernels loaded
            for suffix in (".bai", ".csi"):
                if os.path.exists(path + suffix):
                    os.remove(path + suffix)
            close_time(path, template, records, deflate, leg)
            index = path + (".bai" if leg == "bai" else ".csi")
            files[deflate, leg] = (open(path, "rb").read(), open(index, "rb").read())
        entry["bam_is_one_file_per_deflate"] = (files["device", "bai"][0] == files["device", "csi_host"][0] == files["device", "csi_device"][0]
                                                and files["host", "bai"][0] == files["host", "csi"][0])
        entry["device_fold_equals_host_fold"] = K.inflate(files["device", "csi_device"][1]) == K.inflate(files["device", "csi_host"][1])
        entry["csi_bytes"], entry["bai_bytes"] = len(K.inflate(files["device", "csi_device"][1])), len(files["device", "bai"][1])
        if name == "bam":
            w = B.Written(files["device", "csi_device"][0])
            index = K.read_csi(K.inflate(files["device", "csi_device"][1]))
            K.check_structure(index, w)
            entry["queries_checked"] = K.check_queries(index, w)
            entry["bai_is_the_checkers"] = files["device", "bai"][1] == B.build_bai(w)
        # the tables of the file as written, for the folds alone
        rec_off = np.cumsum([0] + [len(r) for r in records]).astype(np.uint64)
        made, out_off, member_start, spans, _perm, _bad, _kind = nr.bam_sorted_bgzf_device(b"".join(records), rec_off, n_ref, True, "fixed", device)
        del made
        walls = {leg: [] for leg in LEGS}
        kernels, folds = [], {"host_bai_fold_ms": [], "host_csi_fold_ms": [], "device_fold_wall_ms": [], "device_fold_kernels_ms": []}
        for _ in range(reps):
            for deflate, leg in LEGS:
                walls[deflate, leg].append(close_time(path, template, records, deflate, leg) * 1e3)
                if (deflate, leg) == ("device", "csi_device"):
                    kernels.append(dict(nr.bam_index_last_times(), **{"deflate_" + k: v for k, v in nr.bgzf_deflate_last_times().items()}))
            for key, fold in (("host_bai_fold_ms", lambda: nr.bai_build(spans, n_ref, member_start, out_off)),
                              ("host_csi_fold_ms", lambda: nr.csi_build_bam(spans, n_ref, l_ref_max, member_start, out_off)),
                              ("device_fold_wall_ms", lambda: nr.csi_build_bam(spans, n_ref, l_ref_max, member_start, out_off, device=device))):
                t0 = time.perf_counter()
                fold()
                folds[key].append((time.perf_counter() - t0) * 1e3)
            t = nr.bam_index_last_times()
            folds["device_fold_kernels_ms"].append(sum(v for k, v in t.items() if k.endswith("kernel_s")) * 1e3)
        for deflate in ("device", "host"):
            entry[deflate] = {leg: {"wall_ms": median_ms(walls[d, leg])} for d, leg in LEGS if d == deflate}
            base = entry[deflate]["bai"]["wall_ms"]["median"]
            for leg in entry[deflate]:
                entry[deflate][leg]["over_bai"] = entry[deflate][leg]["wall_ms"]["median"] / base
        entry["folds_alone"] = {k: median_ms(v) for k, v in folds.items()}
        entry["folds_alone"]["host_csi_over_device_wall"] = entry["folds_alone"]["host_csi_fold_ms"]["median"] / entry["folds_alone"]["device_fold_wall_ms"]["median"]
        entry["device"]["csi_device"]["runs"], entry["device"]["csi_device"]["passes"] = kernels[0]["runs"], kernels[0]["passes"]
        entry["device"]["csi_device"]["kernels_ms_median"] = {k[:-2] + "_ms": statistics.median(t[k] for t in kernels) * 1e3 for k in kernels[0] if k.endswith("kernel_s")}
        entry["device"]["csi_device"]["fold_total_ms_median"] = statistics.median(t["total_s"] for t in kernels) * 1e3
        close = entry["device"]
        entry["fold_share_of_close"] = {"host_csi": entry["folds_alone"]["host_csi_fold_ms"]["median"] / close["csi_host"]["wall_ms"]["median"],
                                        "device_csi": close["csi_device"]["fold_total_ms_median"] / close["csi_device"]["wall_ms"]["median"],
                                        "host_bai": entry["folds_alone"]["host_bai_fold_ms"]["median"] / close["bai"]["wall_ms"]["median"]}
        result[name] = entry
template.close()
print(json.dumps(result, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")

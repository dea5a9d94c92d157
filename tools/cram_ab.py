#!/usr/bin/env python
"""What reading CRAM costs, in ONE process, legs interleaved, --reps timed runs (default 5) after one untimed run each, medians
with ranges.  The fixture BAM is written as CRAM 3.0 by tests/cramwriter.py (external blocks, rANS order 0 and order 1 by
series, 1 000 records per slice).

(a) rANS batch decode (cram.rans_decode): the host twin on this process's CPUs against the device entry with its transfers
    (wall) and its kernels alone (HIP events), over
      fixture      the rANS blocks of the fixture's CRAM
      fixture_x    --copies (default 50) copies of the fixture with a copy's reads renamed by its number, as one CRAM
      one_order1   ONE order-1 block alone: the shape the four-lanes-per-block design is worst at
    as uncompressed bytes per second, and the kernels' share of a device-to-device copy of 256 MiB measured in the same run.
(b) end to end, singlesample.sso_genotype over the fixture and tests/data/example.vcf: `.bam` with the native reader and with the
    Python reader, `.cram` with cram_codec host and device; and where a whole-file walk of the CRAM spends its time: block decode,
    slice decode, Python record objects.

--work DIR keeps the two CRAMs from run to run.  Writes one JSON object to --out (default profiles/cram_ab.json) and prints it.
GPU box only."""
import io
import json
import os
import socket
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cramwriter as cw  # noqa: E402
from svtyper_amd import bam, cram, singlesample  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps = int(arg("--reps", 5))
copies = int(arg("--copies", 50))
device = int(arg("--device", 0))
out_path = arg("--out", os.path.join(ROOT, "profiles", "cram_ab.json"))
work = arg("--work", None)      # a directory that keeps the two CRAMs from run to run (writing the large one takes minutes of Python)
DATA = os.path.join(ROOT, "tests", "data")
FIXTURE, VCF, LIB_JSON = (os.path.join(DATA, n) for n in ("NA12878.target_loci.sorted.bam", "example.vcf", "NA12878.bam.json"))


def fixture_records():
    f = bam.AlignmentFile(FIXTURE)
    out = []
    f._bgzf.seek(f._first_record)
    while True:
        r = f._next_record()
        if r is None:
            break
        out.append(r._raw)
    text = f.text
    f.close()
    return text, out


def renamed(raw: bytes, k: int) -> bytes:
    """the record with the copy's number in front of its read name"""
    l_name = raw[8]
    name = b"%d." % k + raw[32:32 + l_name]
    if len(name) > 255:
        name = name[:254] + b"\0"
    return raw[:8] + bytes([len(name)]) + raw[9:32] + name + raw[32 + l_name:]


def rans_blocks(path):
    """(blocks, output sizes) of every rANS block of the CRAM"""
    f = cram.CramFile(path)
    blocks, sizes = [], []
    at = f._first
    while True:
        c = f._container(at)
        if c is None or f._is_eof(c):
            break
        at = c.end
        for b in f._blocks(c):
            if b.method == 4:
                blocks.append(bytes(b.data))
                sizes.append(b.raw_size)
    f.close()
    return blocks, sizes


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


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


def rans_leg(blocks, sizes, copy_rate):
    total = sum(sizes)
    walls = {"host": [], "device": []}
    kernels, uploads, downloads = [], [], []
    ref = None
    for rep in range(reps + 1):
        for codec in ("host", "device"):
            t0 = time.perf_counter()
            out, _off, status = cram.rans_decode(blocks, sizes, codec, device)
            wall = time.perf_counter() - t0
            assert not status.any()
            if ref is None:
                ref = out.tobytes()
            assert out.tobytes() == ref
            if rep:
                walls[codec].append(wall)
                if codec == "device":
                    t = cram.rans_last_times()
                    kernels.append(t["order0_kernel_s"] + t["order1_kernel_s"])
                    uploads.append(t["upload_s"])
                    downloads.append(t["download_s"])
    k = statistics.median(kernels)
    return {"blocks": len(blocks), "order1_blocks": sum(1 for b in blocks if b[0] == 1), "compressed_bytes": sum(len(b) for b in blocks),
            "bytes": total, "host_wall_s": spread(walls["host"]), "device_wall_s": spread(walls["device"]), "device_kernels_s": spread(kernels),
            "device_upload_s": spread(uploads), "device_download_s": spread(downloads),
            "host_bytes_per_s": total / statistics.median(walls["host"]), "device_bytes_per_s": total / statistics.median(walls["device"]),
            "kernel_bytes_per_s": total / k, "kernel_share_of_device_copy": total / k / copy_rate,
            "device_over_host": statistics.median(walls["device"]) / statistics.median(walls["host"]),
            "ranges_apart_for_device": max(walls["device"]) < min(walls["host"])}


def sso(path, **kw):
    out = io.StringIO()
    with open(VCF) as vcf_in, open(os.devnull, "w") as null:
        old, sys.stderr = sys.stderr, null
        try:
            singlesample.sso_genotype(path, vcf_in, out, 20, 1, 1, 1000000, LIB_JSON, False, None, False, 1000, 1e10, None, 1000, **kw)
        finally:
            sys.stderr = old
    return [l for l in out.getvalue().split("\n") if not l.startswith("##fileDate")]


def walk_parts(path):
    """a whole-file walk of the CRAM in its three parts, each timed on its own"""
    f = cram.CramFile(path)
    slices, at = [], f._first
    while True:
        c = f._container(at)
        if c is None or f._is_eof(c):
            break
        at = c.end
        slices.extend(f._slices(c))
    t0 = time.perf_counter()
    pending = []
    for _key, comp, sl, blocks in slices:
        pending.extend([comp, sl] + blocks)
    f._undo(pending)
    t1 = time.perf_counter()
    decoded = [cram.decode_slice(comp.content, sl.content, [(b.cid, b.ctype == 5, b.content) for b in blocks], f._rg_ids, len(f.references))
               for _key, comp, sl, blocks in slices]
    t2 = time.perf_counter()
    n = sum(1 for data, rec_off in decoded for _r in f._records(data, rec_off))
    t3 = time.perf_counter()
    f.close()
    return {"records": n, "block_decode_s": t1 - t0, "slice_decode_s": t2 - t1, "record_objects_s": t3 - t2}


def main():
    report = {"reps": reps, "copies": copies, "device": device, "box": socket.gethostname(), "cpus": len(os.sched_getaffinity(0))}
    text, records = fixture_records()
    tmp = work or tempfile.mkdtemp(prefix="cram_ab_")
    os.makedirs(tmp, exist_ok=True)
    path = os.path.join(tmp, "fixture.cram")
    if not os.path.exists(path):
        cw.write_cram(path, text, records, cw.default_layout())
    report["fixture"] = {"records": len(records), "bam_bytes": os.path.getsize(FIXTURE), "cram_bytes": os.path.getsize(path)}
    big = os.path.join(tmp, "fixture_x%d.cram" % copies)
    if not os.path.exists(big):
        cw.write_cram(big, text, [renamed(r, k) for k in range(copies) for r in records], cw.default_layout(), crai=False)
    copy_rate = device_copy_rate()
    report["device_copy_bytes_per_s"] = copy_rate
    blocks, sizes = rans_blocks(path)
    legs = {"fixture": rans_leg(blocks, sizes, copy_rate)}
    legs["fixture_x"] = rans_leg(*rans_blocks(big), copy_rate)
    k = max((i for i, b in enumerate(blocks) if b[0] == 1), key=lambda i: sizes[i])
    legs["one_order1"] = rans_leg([blocks[k]], [sizes[k]], copy_rate)
    report["rans"] = legs
    # (b) end to end
    runs = {"bam_native": lambda: sso(FIXTURE, reader="native"), "bam_python": lambda: sso(FIXTURE, reader="python"),
            "cram_host": lambda: sso(path, cram_codec="host"), "cram_device": lambda: sso(path, cram_codec="device")}
    want = None
    walls = {name: [] for name in runs}
    for rep in range(reps + 1):
        for name, fn in runs.items():
            t0 = time.perf_counter()
            got = fn()
            wall = time.perf_counter() - t0
            want = got if want is None else want
            assert got == want, name
            if rep:
                walls[name].append(wall)
    e2e = {name: spread(w) for name, w in walls.items()}
    for name in ("cram_host", "cram_device"):
        e2e[name + "_over_bam_python"] = e2e[name]["median"] / e2e["bam_python"]["median"]
    e2e["walk_parts_host_codec"] = walk_parts(path)
    report["end_to_end"] = e2e
    text_out = json.dumps(report, indent=1, sort_keys=True)
    with open(out_path, "w") as f:
        f.write(text_out + "\n")
    print(text_out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Corrupted BAMs (bit flips, truncation, overwritten spans) through the native reader, one subprocess each: the
reader must answer with an error (or a result), never crash.  `--walk` (or SVT_FUZZ_WALK=1): the same corpus also goes to
svt_bam_evidence_walk_host, the one-source evidence walk without a fallback, against svt_bam_evidence: it must never crash,
and wherever the host reader succeeds every unit the walk does not flag must carry the host reader's records.
`--inflate` (or SVT_FUZZ_INFLATE=1): the corruption goes into the compressed payload bytes of the BGZF members only (headers and
trailers stay whole), every member goes through the one-source decoder (svt_bgzf_inflate_host) whose verdict must be raw zlib's,
and the file goes through svt_bam_evidence_walk_open_host (the inflate="device" route without a GPU) under the walk's rule."""
import os, sys, subprocess, tempfile, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
child = r'''
import sys, json, os
ROOT = os.environ["SVT_ROOT"]; sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import test_native_reads as N
from svtyper_amd import bam, library, native_reads as nr, hip
path = sys.argv[1]
info = json.load(open(sys.argv[2]))
sites = json.load(open(sys.argv[3]))
try:
    nb = nr.NativeBam(path)
    pybam = bam.AlignmentFile(sys.argv[4])           # the intact copy, for the library / windows only
    sample = library.Sample.from_lib_info(pybam, info, 1e-3)
    walks = []
    if os.environ.get("SVT_FUZZ_WALK") == "1":
        walks.append(nb.evidence_walk_host)
    if os.environ.get("SVT_FUZZ_INFLATE") == "1":
        import inflatecases as I
        data = open(path, "rb").read()
        block_off, out_off = nr.bgzf_members(data)
        out, status = nr.bgzf_inflate(data, block_off, out_off)
        ends = list(block_off[1:]) + [int(block_off[-1]) + (data[int(block_off[-1]) + 16] | data[int(block_off[-1]) + 17] << 8) + 1] if len(block_off) else []
        I.check_against_reference([("member%d" % k, data[int(block_off[k]):int(ends[k])]) for k in range(len(block_off))], out, status, out_off)
        walks.append(nb.evidence_walk_open_host)
    for walk in walks:
        import walkcases as W
        for mode, limit in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 150)):
            a = W.unit_arrays(sites, sample, nb, mode)
            got = walk(a[0], a[1], a[2], a[3], limit, mode, a[4], 20, 3, 2)
            try:
                want = nb.evidence(a[0], a[1], a[2], a[3], limit, mode, a[4], 20, 3, 2)
            except hip.SvtyperHipError:
                assert got[3].any(), "the host reader fails and the walk flags nothing"
                continue
            for u in range(len(sites)):
                if got[3][u]:
                    assert got[0][u + 1] == got[0][u]
                    continue
                assert got[2][u] == want[2][u], "skip flag of unit %d" % u
                assert got[1][int(got[0][u]):int(got[0][u + 1])].tobytes() == want[1][int(want[0][u]):int(want[0][u + 1])].tobytes(), "records of unit %d" % u
    N._native_summaries(sites, sample, nb, nr.COUNT_CLASSIC, None, 2)
    print("ok")
except hip.SvtyperHipError as e:
    print("error:", str(e)[:80])
'''
if "--walk" in sys.argv[1:]:
    os.environ["SVT_FUZZ_WALK"] = "1"
if "--inflate" in sys.argv[1:]:
    os.environ["SVT_FUZZ_INFLATE"] = "1"
tmp = tempfile.mkdtemp()
import test_native_reads as N, json
good = os.path.join(tmp, "good.bam")
sites, info = N._synthetic_bam(good, seed=77, n_pairs=300)
json.dump(info, open(os.path.join(tmp, "info.json"), "w")); json.dump(sites, open(os.path.join(tmp, "sites.json"), "w"))
raw = open(good, "rb").read(); bai = open(good + ".bai", "rb").read()
rng = random.Random(5)
payload_bytes = []      # --inflate: the positions of the compressed payloads
if os.environ.get("SVT_FUZZ_INFLATE") == "1":
    at = 0
    while at + 18 <= len(raw):
        size = (raw[at + 16] | raw[at + 17] << 8) + 1
        payload_bytes += range(at + 18, at + size - 8)
        at += size
outcomes = {}
for it in range(int(os.environ.get('SVT_FUZZ_ITERS', '60'))):
    b = bytearray(raw)
    mode = it % 3
    if payload_bytes:
        if mode == 0:
            for _ in range(rng.randint(1, 8)): b[rng.choice(payload_bytes)] ^= 1 << rng.randrange(8)
        elif mode == 1:
            b[rng.choice(payload_bytes)] = rng.randrange(256)
        else:
            p = rng.randrange(len(payload_bytes) - 8)
            for q in payload_bytes[p:p + rng.randint(2, 8)]: b[q] = rng.randrange(256)
    elif mode == 0:
        for _ in range(rng.randint(1, 8)): b[rng.randrange(200, len(b))] ^= 1 << rng.randrange(8)
    elif mode == 1:
        b = b[: rng.randrange(300, len(b))]
    else:
        p = rng.randrange(200, len(b) - 64); b[p:p + 32] = bytes(rng.randrange(256) for _ in range(32))
    bad = os.path.join(tmp, "bad%d.bam" % it)
    open(bad, "wb").write(bytes(b)); open(bad + ".bai", "wb").write(bai)
    r = subprocess.run([sys.executable, "-c", child, bad, os.path.join(tmp, "info.json"), os.path.join(tmp, "sites.json"), good],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, SVT_ROOT=ROOT))
    key = "crash rc=%d" % r.returncode if r.returncode != 0 else r.stdout.strip().split(":")[0]
    outcomes[key] = outcomes.get(key, 0) + 1
    if r.returncode != 0: print(it, mode, r.stderr[-300:])
print(outcomes)
if any(k.startswith("crash") for k in outcomes):
    sys.exit(1)

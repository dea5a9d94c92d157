"""The per-record verdicts of svt_batch_verdicts (include/svtyper_hip.h, bits 0-5) restated in Python -- TEST INFRASTRUCTURE.

Statement for statement after the reference's tagging branches (svtyper/classic.py:317-408, parsers.py:771-782,1218-1228) over
the evidence records, with oracle.py_oracle.p_concordant and prob_mapq: what the kernel bytes are compared with
(tests/test_verdicts_device.py), and what stands in for the device behind `svtyper -w` on a machine without one
(tests/test_write_alignment_host.py: VerdictOracleEngine).  Also the synthetic batches of the device test and the reader of
tests/golden/write_alignment.json.gz.
"""
import gzip
import json
import os

import numpy as np

from oracle.py_oracle import _Lib, p_concordant, prob_mapq
from svtyper_amd import evidence as ev
from svtyper_amd.evidence import EvidenceBatch, LibraryTable, RECORD_DTYPE, UNIT_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))

ALT_TAKEN, ALT_A, REF_TAKEN, REF_A, SEQ_ALT, CLIP_ALT = 1, 2, 4, 8, 16, 32


def restate(batch: EvidenceBatch) -> np.ndarray:
    """one byte per record of `batch`"""
    libs = [_Lib(t) for t in batch.libs]
    out = np.zeros(batch.n_records, np.uint8)
    offs = batch.rec_offset.tolist()
    recs = batch.records.tolist()
    for u in range(batch.n_units):
        unit = batch.units[u]
        if unit["flags"] & ev.UNIT_SKIP:                               # classic.py:282-284
            continue
        is_del = unit["svtype"] == 0
        var_length = int(unit["var_length"]) if is_del else None
        pos_delta = int(unit["pos_delta"])
        for r in range(offs[u], offs[u + 1]):
            (ospan, mq_a, mq_b, _rs_a, _rs_b, seq_l, seq_r, clip_l, clip_r, flags) = recs[r]
            v = 0
            if (prob_mapq(seq_l) + prob_mapq(seq_r)) / 2.0 > 0:      # classic.py:324,330
                v |= SEQ_ALT
            if (prob_mapq(clip_l) + prob_mapq(clip_r)) / 2.0 > 0:
                v |= CLIP_ALT
            if not (flags & ev.REC_CONTINUATION) and flags & ev.REC_HAS_PAIR:
                lib = libs[(flags >> ev.REC_LIB_SHIFT) & 0xFFFF]
                small_del = is_del and pos_delta < 2 * lib.sd           # classic.py:339,383
                alt = (not small_del) and bool(flags & ev.REC_ALT_STRADDLE)
                if alt:                                                 # classic.py:359-380
                    if is_del:
                        p_alt = (1 - p_concordant(lib, ospan, var_length)) * prob_mapq(mq_a) * prob_mapq(mq_b)
                    else:
                        p_alt = prob_mapq(mq_a) * prob_mapq(mq_b)
                    v |= ALT_TAKEN | (ALT_A if p_alt > 0 else 0)
                ra = (not small_del) and bool(flags & ev.REC_REF_STRADDLE_A)
                rb = (not small_del) and bool(flags & ev.REC_REF_STRADDLE_B)
                if (ra or rb) and (not (ra and rb) or is_del):          # classic.py:398-408
                    p_conc = p_concordant(lib, ospan, var_length)
                    v |= REF_TAKEN | (REF_A if 1 - p_conc > 0 else 0)
            out[r] = v
    return out


class VerdictOracleEngine:
    """the C oracle for the result records plus restate() for the verdicts: the engine seam of `svtyper -w` without a GPU"""
    supports_verdicts = True

    def __call__(self, batch, flags=0, verdicts=False):
        from oracle import c_oracle
        res = c_oracle.genotype_batch(batch, flags=flags)
        if verdicts:
            res.verdicts = restate(batch)
        return res


# ------------------------------------------------------------------------------------------ the golden of `svtyper -w`
def golden_cases():
    """tests/golden/write_alignment.json.gz (tests/golden/make_golden_write_alignment.py): per case "writes" -- what the reference
    handed to its output BAM, in order, [query_name, flag, reference_id, reference_start, XV or None] each -- and "mapq", the
    MAPQ of each of them.  A case whose lists equal another case's is stored as {"same_as": that case}."""
    with gzip.open(os.path.join(HERE, "golden", "write_alignment.json.gz"), "rb") as f:
        cases = json.loads(f.read().decode())
    return {name: cases[c["same_as"]] if "same_as" in c else c for name, c in cases.items()}


def written_records(path):
    """(writes, mapq) of a BAM `svtyper -w` wrote, in the golden's form, read with the project's reader, every CRC32 checked"""
    from svtyper_amd.bam import AlignmentFile
    f = AlignmentFile(path, "rb", verify=True)
    f._bgzf.seek(f._first_record)
    writes, mapq = [], []
    while True:
        r = f._next_record()
        if r is None:
            break
        writes.append([r.query_name, r.flag, r.reference_id, r.reference_start, r.get_tag("XV") if r.has_tag("XV") else None])
        mapq.append(r.mapping_quality)
    f.close()
    return writes, mapq


# ------------------------------------------------------------------------------------------ synthetic batches
def _library(rng, k, integral_every):
    """a library whose histogram has holes (hist == 0 -> thr -1); mean + 3 sd is integral for every `integral_every`-th one (then
    the float Counter key of a non-DEL unit can hit a bin, parsers.py:874-878), else never"""
    n_bins = int(rng.integers(40, 90))
    key_min = int(rng.integers(150, 260))
    hist = rng.integers(0, 60, n_bins).astype(np.uint32)
    hist[rng.integers(0, n_bins, 6)] = 0
    hist[n_bins // 2] = 500
    integral = integral_every and k % integral_every == 0
    sd = float(rng.integers(8, 30)) + (0.0 if integral else 0.37)
    mean = float(key_min + n_bins // 2) + (0.0 if integral else 0.21)
    return LibraryTable(hist, key_min, mean, sd, "lib%d" % k)


def _record(rng, lib, table, shift):
    """one first record of library `lib`: spans inside the histogram, at its edges, beyond them (the sentinel bin), and spans whose
    second key (o - `shift`) lies inside it"""
    kind = int(rng.integers(0, 6))
    lo, hi = table.key_min, table.key_min + len(table.hist) - 1
    ospan = (int(rng.integers(lo, hi + 1)), lo, hi, hi + 1 + int(rng.integers(0, 5000)), max(0, lo - 1 - int(rng.integers(0, 100))),
             int(rng.integers(lo, hi + 1)) + shift)[kind]
    mq = lambda: int(rng.choice([0, 0, 1, 20, 37, 60, 255]))
    has_pair = rng.random() < 0.9
    flags = (lib << ev.REC_LIB_SHIFT) | (ev.REC_HAS_PAIR | int(rng.integers(0, 8)) if has_pair else 0)
    return (ospan, mq() if has_pair else 0, mq() if has_pair else 0, mq(), mq(), mq() if rng.random() < 0.3 else 0,
            mq() if rng.random() < 0.3 else 0, mq() if rng.random() < 0.2 else 0, mq() if rng.random() < 0.2 else 0, flags)


def synthetic_batch(n_libs=300, sizes=(0, 1, 63, 64, 65, 129), seed=5, hints=True, integral_every=3):
    """`n_libs` libraries, one sample each.  Per library a DEL unit on either side of 2 * sd (the small-deletion gate) and a non-DEL
    unit; the units' record counts cycle through `sizes`; the first and the last unit are empty, one unit in the middle (with
    records) is skipped.  Records name their unit's library, continuation records (split candidates only) included."""
    rng = np.random.default_rng(seed)
    libs = [_library(rng, k, integral_every) for k in range(n_libs)]
    units, rows, offs = [], [], [0]

    def add_unit(lib, svtype, pos_delta, var_length, n, skip=False):
        u = np.zeros(1, UNIT_DTYPE)
        u["svtype"], u["pos_delta"], u["var_length"] = svtype, pos_delta, var_length if svtype == 0 else 0
        u["sample"] = lib & 0xFFFF
        u["flags"] = ev.UNIT_SKIP if skip else 0
        u["libs"] = ev.unit_libs(lib, 1) if hints else 0
        units.append(u)
        t = libs[lib]
        v = t.mean + t.sd * 3
        shift = var_length if svtype == 0 else int(v)
        end = len(rows) + n
        while len(rows) < end:
            rows.append(_record(rng, lib, t, shift))
            if rng.random() < 0.15 and len(rows) < end:
                rows.append((0, 0, 0, int(rng.choice([0, 30])), 0, int(rng.choice([0, 40])), 0, 0, int(rng.choice([0, 50])),
                             (lib << ev.REC_LIB_SHIFT) | ev.REC_CONTINUATION))
        offs.append(len(rows))

    add_unit(0, 0, 1000, 1000, 0)                         # empty first unit
    k = 0
    for lib in range(n_libs):
        sd2 = 2 * libs[lib].sd
        below = int(np.floor(sd2)) - (1 if sd2 == np.floor(sd2) else 0)      # pos_delta < 2 sd: gated
        for svtype, delta in ((0, below), (0, int(np.ceil(sd2))), (int(rng.integers(1, 4)), 5000)):
            n = sizes[k % len(sizes)]
            k += 1
            skip = lib == n_libs // 2 and svtype != 0
            add_unit(lib, svtype, delta, int(rng.integers(20, 80)), max(n, 5) if skip else n, skip=skip)
    add_unit(n_libs - 1, 2, 10, 0, 0)                     # empty last unit
    rec = np.zeros(len(rows), RECORD_DTYPE)
    if rows:
        arr = np.asarray(rows, dtype=np.int64)
        for i, name in enumerate(RECORD_DTYPE.names):
            rec[name] = arr[:, i]
    return EvidenceBatch(np.asarray(offs, np.uint64), np.concatenate(units), rec, libs)

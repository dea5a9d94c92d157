"""The lattice of the concordance decision -- TEST INFRASTRUCTURE.

The reference decides one boolean per fragment, SamFragment.p_concordant (svtyper/parsers.py:861-882); the device asks
`rank(hist[o - v]) <= rank(thr[o])` of tables that build_tables makes (svtyper_amd/csrc/svt_host_tables.h).  This file names
library families that stand on both sides of every edge of that construction and, per library, the points (ospan_len,
var_length or None) at which the reference is asked (tests/golden/make_golden_concordance.py writes its answers to
tests/golden/concordance_edges.json.gz; the tests believe that file, not this one).  Pure Python and deterministic.

Every library has 2 * sd below 10, so that a DEL unit with pos_delta = POS_DELTA is never behind the small-deletion gate
(classic.py:339), and a non-integral mean + 3 sd unless its name says otherwise.

It also holds the file's own restatement of the threshold search (thresholds, dense_ranks: what the host-table test compares
build_tables with and what places the wide libraries at the limits), and the probe and mixed batches of the host and device
tests.
"""
import functools
import hashlib
import random

import numpy as np

from svtyper_amd import evidence as ev
from svtyper_amd.evidence import EvidenceBatch, LibraryTable, RECORD_DTYPE, UNIT_DTYPE

SEED = 20261019
POS_DELTA = 10_000
MEAN, SD = 300.21, 3.37                 # mean + 3 sd = 310.32
INT31 = 2 ** 31 - 1
SMALL_FAMILIES = ("ratio", "capped", "tiny", "flat", "sparse", "huge", "negative", "nondel")

# the limits svt_batch_create.h sets for one library (create_stream): 16-bit ranks need at most 32 767 distinct values of
# hist + thr + {0} (build_tables: narrow_bins), and the one-library LDS mode needs kSBins + 4 (n_bins + 1) bytes of tables beside
# four 8 KiB rings in 96 KiB
NARROW_VALUES = 32767
K_SBINS = 2 * 256 * 8 + 2 * 32 * 8 + 2 * 32 * 4                      # svt_wg_parts.h: kSBins
LDS_MAX_BINS = (96 * 1024 - 4 * 64 * 128 - K_SBINS) // 4 - 1          # 15 167
ONE_LIBRARY, WINDOWS, GENERAL = 0, 1, 2                               # DeviceBatch.table_mode()


# ------------------------------------------------------------------------------------------ the expression, restated
def expr(h1, h2, n):
    """parsers.py:878-882 for counts h1 = hist[o], h2 = hist[o - v] of a library of n samples (Python floats)"""
    d1 = float(h1) / n if h1 else 0
    d2 = float(h2) / n if h2 else 0
    try:
        p = float(d1) * 0.95 / (0.95 * d1 + 0.05 * d2)
    except ZeroDivisionError:
        return False
    return p > 0.5


def _expr_np(h1, h2, n):
    """expr over arrays of counts (binary64, the same operations in the same order); h1 > 0 everywhere"""
    d1 = h1.astype(np.float64) / float(n)
    d2 = h2.astype(np.float64) / float(n)
    return d1 * 0.95 / (0.95 * d1 + 0.05 * d2) > 0.5


def thresholds(counts):
    """per bin the largest h2 in [0, max count] for which expr(count, h2) holds, -1 where none does (a count of 0): found by
    bisection on the expression itself -- every operation in it rounds monotonically, so it is non-increasing in h2"""
    counts = np.asarray(counts, dtype=np.int64)
    n, hmax = int(counts.sum()), int(counts.max())
    thr = np.full(counts.shape, -1, np.int64)
    live = np.nonzero(counts > 0)[0]
    if live.size == 0:
        return thr
    h1 = counts[live]
    lo = np.zeros(live.size, np.int64)                  # expr(h1, 0) holds for h1 > 0
    hi = np.full(live.size, hmax + 1, np.int64)         # one beyond the range: treated as "does not hold"
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        ok = _expr_np(h1, mid, n)
        lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
    thr[live] = lo
    return thr


def dense_ranks(counts):
    """(thr_rank, hist_rank, distinct values): counts and thresholds by their rank among the distinct values of
    counts + thresholds + {0}; -1 stays -1; the last entry of both is the out-of-range sentinel (-1, rank of 0)"""
    counts = np.asarray(counts, dtype=np.int64)
    thr = thresholds(counts)
    vals = np.unique(np.concatenate([counts, thr[thr >= 0], [0]]))
    hist_rank = np.append(np.searchsorted(vals, counts), 0)
    thr_rank = np.append(np.where(thr >= 0, np.searchsorted(vals, np.maximum(thr, 0)), -1), -1)
    return thr_rank, hist_rank, int(vals.size)


# ------------------------------------------------------------------------------------------ libraries
class Lib:
    def __init__(self, family, name, hist, mean=MEAN, sd=SD, points=None):
        self.family, self.name, self.hist, self.mean, self.sd = family, name, dict(hist), float(mean), float(sd)
        self.points = pair_points(self.hist) if points is None else points
        assert 2 * self.sd < 10 or family == "nondel"

    def table(self):
        return LibraryTable.from_counter(self.hist, self.mean, self.sd, self.name)


def _run(key, counts):
    return {key + i: int(c) for i, c in enumerate(counts)}


def pair_points(hist, b_keys=None):
    """every ordered pair (a, b) of the keys from one below the histogram to one above it: ospan_len = a (a span is never
    negative), var_length = a - b, of both signs and 0"""
    lo, hi = min(hist) - 1, max(hist) + 1
    keys = range(lo, hi + 1)
    return [(a, a - b) for a in keys if a >= 0 for b in (keys if b_keys is None else b_keys)]


def _ratio_hist(h1, n):
    counts = [0, h1, 19 * h1 - 2, 19 * h1 - 1, 19 * h1, 19 * h1 + 1, 19 * h1 + 2, 0, 1, h1]   # [0]: the padding bin
    counts[0] = n - sum(counts)
    assert 0 <= counts[0] <= INT31
    return _run(200, counts)


def ratio_pairs():
    """[(h1, N, expr at h2 = 19 h1)]: the pair of the issue first, then a seeded search until four of either answer"""
    out = [(1817, 1872973, expr(1817, 19 * 1817, 1872973))]
    rng = random.Random(SEED)
    want = {True: 4, False: 4}
    want[out[0][2]] -= 1
    while want[True] or want[False]:
        h1 = rng.randint(1, 3000)
        n = rng.randint(200 * h1 + 10, 4_000_000)
        at = expr(h1, 19 * h1, n)
        if want[at]:
            want[at] -= 1
            out.append((h1, n, at))
    return out


def _nondel(name, mean, sd):
    """two clusters mean + 3 sd apart (282 when that is integral): 19 : 1 bins across them"""
    low = [19 * 7 - 1, 19 * 7, 19 * 7 + 1, 0, 40]
    high = [7, 7, 7, 3, 40]
    hist = _run(100, low)
    hist.update(_run(382, high))
    spans = sorted(set(list(range(99, 106)) + list(range(381, 388)) + [0, 1, 281, 282, 283, 664, 665, 2 ** 30, 2 ** 30 + 382,
                                                                     INT31 - 1, INT31]))
    return Lib("nondel", name, hist, mean, sd, [(o, None) for o in spans])


@functools.lru_cache(maxsize=None)
def small_libraries():
    """the libraries whose histograms, points and answers the golden stores, in order"""
    libs = []
    for k, (h1, n, at) in enumerate(ratio_pairs()):
        libs.append(Lib("ratio", "ratio%d_%s" % (k, "true" if at else "false"), _ratio_hist(h1, n)))
    # capped: 19 h1 > hmax = 1000 for h1 >= 53, so the threshold is hmax itself; hist[o - v] = hmax is equality at the cap
    libs.append(Lib("capped", "capped", _run(250, [100, 1000, 60, 52, 53, 0, 1, 999, 1000, 54])))
    libs.append(Lib("tiny", "tiny_1", {275: 1}))
    for c in (18, 19, 20):
        libs.append(Lib("tiny", "tiny_1_%d" % c, {275: 1, 276: c}))
    for c in (37, 38, 39):
        libs.append(Lib("tiny", "tiny_2_%d" % c, {275: 2, 276: c}))
    libs.append(Lib("flat", "flat", _run(280, [7] * 50)))
    libs.append(Lib("sparse", "sparse", _run(300, [5, 0, 0, 95, 0, 100, 0, 1, 19, 0, 0, 2, 38, 0, 3, 57, 56, 0, 0, 4])))
    q = INT31 // 19
    libs.append(Lib("huge", "huge", _run(290, [INT31, INT31, INT31, q - 2, q - 1, q, q + 1, q + 2, 0, 1, INT31 - 1])))
    wave = [1 + (k * k) % 23 + (19 * 12 if k % 9 == 0 else 0) for k in range(81)]
    wave[10], wave[50], wave[70] = 0, 0, 12
    wave[20], wave[21], wave[22] = 19 * 12 - 1, 19 * 12, 19 * 12 + 1
    libs.append(Lib("negative", "negative_m40", _run(-40, wave)))
    for key_min in (-2 ** 29 - 1, -2 ** 29, 2 ** 29, 2 ** 29 + 1):
        hist = _run(key_min, [5, 95, 1, 0, 100])
        if key_min < 0:      # no span reaches a bin: the bins are seen only as hist[o - v]
            points = [(o, o - b) for o in (0, 1, 5, 1000) for b in range(key_min - 1, key_min + 6)]
        else:
            points = pair_points(hist)
        libs.append(Lib("negative", "keymin_%s%d" % ("m" if key_min < 0 else "p", abs(key_min)), hist, points=points))
    libs.append(_nondel("nondel_integral", 270.0, 4.0))
    libs.append(_nondel("nondel_3e-6", 270.000003, 4.0))
    libs.append(_nondel("nondel_5e-6", 270.000005, 4.0))
    assert len({L.name for L in libs}) == len(libs)
    return tuple(libs)


def family(name):
    return [L for L in small_libraries() if L.family == name]


# ------------------------------------------------------------------------------------------ the wide family
WIDE_KEY_MIN = 100
WIDE_RECIPES = ("wide_values_32767", "wide_values_32768", "wide_bins_lds_fit", "wide_bins_lds_over")


def _wide_counts(n_bins, extra=()):
    """20, 40, ..., 20 n_bins (bin 19 k - 1 holds 19 times what bin k - 1 holds: the boundary itself), then `extra`"""
    return np.concatenate([20 * np.arange(1, n_bins + 1, dtype=np.int64), np.asarray(extra, dtype=np.int64)])


@functools.lru_cache(maxsize=None)
def _values_ramp():
    n = 31100
    assert dense_ranks(_wide_counts(n))[2] < NARROW_VALUES - 3
    while dense_ranks(_wide_counts(n))[2] < NARROW_VALUES:
        n += 1
    return n - 3


@functools.lru_cache(maxsize=None)
def wide_counts(recipe):
    """the histogram (int64 array, key WIDE_KEY_MIN first) of a wide library.  The two `values` libraries are a ramp three bins
    short of the one at which this file's own threshold search first finds 32 767 distinct values, and behind it bins with
    counts just below the largest, each the first that adds exactly one value, until there are 32 767 / 32 768 of them."""
    if recipe == "wide_bins_lds_fit":
        return _wide_counts(LDS_MAX_BINS)
    if recipe == "wide_bins_lds_over":
        return _wide_counts(LDS_MAX_BINS + 1)
    n = _values_ramp()
    target = NARROW_VALUES + (recipe == "wide_values_32768")
    assert recipe in ("wide_values_32767", "wide_values_32768")
    extra, t = [], 0
    have = dense_ranks(_wide_counts(n))[2]
    while have < target:
        t += 1
        assert t < 400, "no extra bin adds one value"
        if t % 20 and dense_ranks(_wide_counts(n, extra + [20 * n - t]))[2] == have + 1:
            extra.append(20 * n - t)
            have += 1
    return _wide_counts(n, extra)


def wide_sha256(recipe):
    return hashlib.sha256(wide_counts(recipe).astype("<u4").tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def wide_library(recipe):
    counts = wide_counts(recipe)
    n = len(counts)
    rng = random.Random(SEED + WIDE_RECIPES.index(recipe))
    top = list(range(n - 20, n))
    low = list(range(10))
    pairs = [(a, b) for a in top for b in top]                       # the highest ranks on both sides
    pairs += [(a, b) for a in low for b in top] + [(a, b) for a in top for b in low]
    for k in sorted(rng.sample(range(1, n // 19), 300)):             # bin k - 1 against the bins around 19 times its count
        pairs += [(k - 1, 19 * k - 2), (k - 1, 19 * k - 1), (k - 1, 19 * k)]
    pairs += [(rng.randrange(n), rng.randrange(-1, n + 1)) for _ in range(300)]
    pairs += [(n, n - 1), (n - 1, n), (n - 1, -1), (0, -1), (0, 0), (n - 1, n - 1)]
    points = [(WIDE_KEY_MIN + a, a - b) for a, b in pairs]
    L = Lib.__new__(Lib)
    L.family, L.name, L.mean, L.sd, L.points = "wide", recipe, MEAN, SD, points
    L.hist = None
    L.counts = counts
    L.table = lambda: LibraryTable(counts.astype(np.uint32), WIDE_KEY_MIN, MEAN, SD, recipe)
    return L


# ------------------------------------------------------------------------------------------ batches
PAIR_FLAGS = ev.REC_HAS_PAIR | ev.REC_ALT_STRADDLE | ev.REC_REF_STRADDLE_A


def _records(rows):
    rec = np.zeros(len(rows), RECORD_DTYPE)
    if rows:
        arr = np.asarray(rows, dtype=np.int64)
        for i, name in enumerate(RECORD_DTYPE.names):
            rec[name] = arr[:, i]
    return rec


def _hint(lib, hints, n_libs):
    """svt_unit.libs of a unit of library `lib`: hints = 0 none, 1 the library alone, w > 1 the aligned group of w libraries
    that holds it (cut at the batch's last library)"""
    w = int(hints)
    if w <= 0:
        return 0
    first = lib - lib % w
    return ev.unit_libs(first, min(w, n_libs - first))


def probe_batch(libs, hints=True, index=None, tables=None, only_nonnegative=False):
    """one unit per point of every library of `libs` (library k of the list is library index[k] of the batch, k without one), exactly one
    record each: HAS_PAIR | ALT_STRADDLE | REF_STRADDLE_A, MAPQ 60 / 60, DEL with the point's var_length -- for a point without
    one REF_STRADDLE_A alone on a DUP, INV or BND unit.  Returns (batch, [(position of the library in libs, point index)])."""
    units, rows, where = [], [], []
    for k, L in enumerate(libs):
        lib = k if index is None else index[k]
        for j, (o, v) in enumerate(L.points):
            if only_nonnegative and v is not None and v < 0:
                continue
            u = np.zeros(1, UNIT_DTYPE)
            u["svtype"] = 0 if v is not None else 1 + j % 3
            u["var_length"] = v if v is not None else 0
            u["pos_delta"] = POS_DELTA
            u["sample"] = lib & 0xFFFF
            u["libs"] = _hint(lib, hints, len(libs) if tables is None else len(tables))
            units.append(u)
            flags = (PAIR_FLAGS if v is not None else ev.REC_HAS_PAIR | ev.REC_REF_STRADDLE_A) | (lib << ev.REC_LIB_SHIFT)
            rows.append((o, 60, 60, 0, 0, 0, 0, 0, 0, flags))
            where.append((k, j))
    tables = [L.table() for L in libs] if tables is None else tables
    return EvidenceBatch(np.arange(len(rows) + 1, dtype=np.uint64), np.concatenate(units), _records(rows), tables), where


def probe_tallies(batch, answers):
    """the five tallies of every unit of a probe batch from the golden booleans alone (`answers`: one per unit)"""
    pm60 = 1 - 10 ** (-60 / 10.0)                                 # utils.py:74-75
    want = np.zeros((batch.n_units, 5), np.float64)
    is_del = batch.units["svtype"] == 0
    conc = np.asarray(answers, dtype=bool)
    want[:, ev.TALLY_NAMES.index("ref_span")] = np.where(conc, pm60 * pm60 / 2, 0.0)
    want[:, ev.TALLY_NAMES.index("alt_span")] = np.where(is_del & ~conc, pm60 * pm60, 0.0)
    return want


MIXED_SIZES = (1, 63, 64, 65, 129, 300)


def mixed_batch(libs, hints=True, index=None, tables=None, seed=0, only_nonnegative=False):
    """units of 1, 63, 64, 65, 129 and 300 records (cycling over the libraries) drawn from the points of one library that share
    a var_length: varied MAPQs (0 and 255 among them), every straddle-bit combination, records without a pair and continuation
    records (split candidates only).  The units stay in front of the small-deletion gate."""
    rng = random.Random(SEED + seed)
    mapqs = (0, 0, 1, 20, 37, 60, 255)
    units, rows, offs = [], [], [0]
    for k, L in enumerate(libs):
        lib = k if index is None else index[k]
        by_v = {}
        for o, v in L.points:
            if not (only_nonnegative and v is not None and v < 0):
                by_v.setdefault(v, []).append(o)
        groups = sorted(by_v.items(), key=lambda kv: (-len(kv[1]), kv[0] if kv[0] is not None else 0))
        for i, size in enumerate(MIXED_SIZES):
            v, spans = groups[(i * 3) % len(groups)]
            u = np.zeros(1, UNIT_DTYPE)
            u["svtype"] = 0 if v is not None else 1 + i % 3
            u["var_length"] = v if v is not None else 0
            u["pos_delta"] = POS_DELTA
            u["sample"] = lib & 0xFFFF
            u["libs"] = _hint(lib, hints, len(libs) if tables is None else len(tables))
            units.append(u)
            end = len(rows) + size
            while len(rows) < end:
                mq = lambda: rng.choice(mapqs)
                pair = rng.random() < 0.9
                flags = (lib << ev.REC_LIB_SHIFT) | ((ev.REC_HAS_PAIR | rng.randrange(8)) if pair else 0)
                rows.append((rng.choice(spans), mq() if pair else 0, mq() if pair else 0, mq(), mq(), mq() if rng.random() < 0.3 else 0,
                             mq() if rng.random() < 0.3 else 0, mq() if rng.random() < 0.2 else 0, mq() if rng.random() < 0.2 else 0, flags))
                if rng.random() < 0.15 and len(rows) < end:
                    rows.append((0, 0, 0, rng.choice((0, 30)), 0, rng.choice((0, 40)), 0, 0, rng.choice((0, 50)),
                                 (lib << ev.REC_LIB_SHIFT) | ev.REC_CONTINUATION))
            offs.append(len(rows))
    tables = [L.table() for L in libs] if tables is None else tables
    return EvidenceBatch(np.asarray(offs, np.uint64), np.concatenate(units), _records(rows), tables)


FILLER = {100: 1, 101: 1}


def with_fillers(libs, n_libs):
    """(tables, index): `libs` split over the lowest and the highest indices of n_libs libraries, two-bin fillers that nobody
    names between them (as manylibcases.highest_library); index[k] = where library k of `libs` went"""
    filler = LibraryTable.from_counter(FILLER, 100.5, 0.7, "filler")
    half = (len(libs) + 1) // 2
    index = list(range(half)) + list(range(n_libs - (len(libs) - half), n_libs))
    tables = [filler] * n_libs
    for k, L in zip(index, libs):
        tables[k] = L.table()
    return tables, index

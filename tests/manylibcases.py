"""Batches of more than 256 libraries for the tests of packed evidence (test_packed_many_libraries_*.py): built once per
process and shared; the tests treat them as read-only (a test that needs a variant copies the arrays it changes)."""
import functools

import numpy as np

from svtyper_amd import evidence as ev
from svtyper_amd import synth


def three_libraries(fixture_library):
    return [fixture_library, synth.normal_library(420.0, 95.0, seed=3), synth.normal_library(270.0, 40.0, seed=5)]


def spread_over_libraries(batch, n_libs, tables):
    """`batch` was made against the three tables; the same units against `n_libs` libraries that cycle the three: sample g
    owns libraries [3 g, 3 g + 3) (the last sample what is left of them), unit u belongs to sample u mod n_samples, and a
    record of table t names the sample's library 3 g + t mod (its count) -- with the window hint on every unit."""
    n_samples = (n_libs + 2) // 3
    g = np.arange(batch.n_units, dtype=np.int64) % n_samples
    count = np.minimum(3, n_libs - 3 * g)
    per_unit = np.diff(batch.rec_offset.astype(np.int64))
    rg, rc = np.repeat(g, per_unit), np.repeat(count, per_unit)
    fl = batch.records["flags"].astype(np.int64)
    lib = 3 * rg + ((fl >> ev.REC_LIB_SHIFT) & 0xffff) % rc
    records = batch.records.copy()
    records["flags"] = ((fl & 0xff) | (lib << ev.REC_LIB_SHIFT)).astype(np.uint32)
    units = batch.units.copy()
    units["libs"] = [ev.unit_libs(3 * int(a), int(c)) for a, c in zip(g, count)]
    units["sample"] = g % 65536
    return ev.EvidenceBatch(batch.rec_offset.copy(), units, records, [tables[k % 3] for k in range(n_libs)],
                            batch.split_weight, batch.disc_weight)


@functools.lru_cache(maxsize=None)
def _many(n_libs, n_units, key):
    tables = _many.tables[key]
    base = synth.make_units(n_units, 1000 + n_libs, tables, svtype_mix=(0.5, 0.2, 0.2, 0.1), mean_frags=20, sd_frags=6, min_frags=0,
                            max_frags=40, frac_empty=0.02, frac_skip=0.01)
    base.records["mapq_a"][::5] = 37           # wide entries behind and in front of switches, every alignment
    return spread_over_libraries(base, n_libs, tables)


_many.tables = {}


def many_libraries(fixture_library, n_libs, n_units):
    """n_units units of ~20 records over n_libs libraries (cycling the fixture's library and two rounded-normal ones)"""
    key = id(fixture_library)
    if key not in _many.tables:
        _many.tables[key] = three_libraries(fixture_library)
    return _many(n_libs, n_units, key)


def interleaved_across_the_boundary(fixture_library, n_libs=300, n_units=600):
    """every unit's records alternate between library 255 (the last the short switch names) and 256 (the first that takes the
    wide one), record by record; a few units use 254 / 257 as well so that a workgroup sees several pairs"""
    tables = three_libraries(fixture_library)
    base = synth.make_units(n_units, 4242, tables, svtype_mix=(0.5, 0.2, 0.2, 0.1), mean_frags=24, sd_frags=8, min_frags=0, max_frags=60)
    base.records["mapq_a"][::4] = 23
    off = base.rec_offset.astype(np.int64)
    unit_of = np.repeat(np.arange(base.n_units), np.diff(off))
    within = np.arange(base.n_records) - off[:-1][unit_of]
    lo = np.where(unit_of % 5 == 0, 254, 255)
    lib = lo + (within % 2) * np.where(unit_of % 5 == 0, 3, 1)        # 255 / 256, every fifth unit 254 / 257
    records = base.records.copy()
    records["flags"] = ((records["flags"].astype(np.int64) & 0xff) | (lib << ev.REC_LIB_SHIFT)).astype(np.uint32)
    units = base.units.copy()
    units["libs"] = ev.unit_libs(254, 4)
    return ev.EvidenceBatch(base.rec_offset.copy(), units, records, [tables[k % 3] for k in range(n_libs)], 1.0, 1.0)


def highest_library(fixture_library, n_units=192):
    """65 536 libraries of which the units name six: 0..2 and 65 533..65 535 (the three tables); the others are two-bin
    fillers nobody names -- what a batch's last sample looks like to the decoder"""
    tables = three_libraries(fixture_library)
    filler = ev.LibraryTable.from_counter({100: 1, 101: 1}, 100.5, 0.7, "filler")
    base = synth.make_units(n_units, 65535, tables, svtype_mix=(0.5, 0.2, 0.2, 0.1), mean_frags=20, sd_frags=6, min_frags=0, max_frags=40)
    base.records["mapq_b"][::6] = 41
    per_unit = np.diff(base.rec_offset.astype(np.int64))
    first = np.where(np.arange(base.n_units) % 2 == 0, 65533, 0)
    fl = base.records["flags"].astype(np.int64)
    lib = np.repeat(first, per_unit) + ((fl >> ev.REC_LIB_SHIFT) & 0xffff)
    records = base.records.copy()
    records["flags"] = ((fl & 0xff) | (lib << ev.REC_LIB_SHIFT)).astype(np.uint32)
    units = base.units.copy()
    units["libs"] = [ev.unit_libs(int(f), 3) for f in first]
    libs = [filler] * 65536
    libs[0:3] = tables
    libs[65533:65536] = tables
    return ev.EvidenceBatch(base.rec_offset.copy(), units, records, libs, 1.0, 1.0)

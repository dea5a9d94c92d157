"""Packed evidence of more than 256 libraries, host side (svt_pack_evidence_flags + SVT_PACK_MANY_LIBRARIES): the pair streams
the encoder writes are read back by a small decoder of this file -- entries, no-ops, short and wide library switches, as
svtyper_amd/csrc/svt_entry_formats.h states them -- and compared with what the canonical records say must be stored; the
slots of batches of at most 256 libraries are the ones the untouched oracle/py_packed.py reads; every form of the encoder
writes the same slots; the limits that stay are still answered as they were."""
import os

import numpy as np
import pytest

from svtyper_amd import evidence as ev
from svtyper_amd import synth

import manylibcases

WIDE = 0x8000            # kWideEntry / kWideSwitch
SHORT_SWITCH_LIBS = 256  # kShortSwitchLibs


def decode_pair_stream(halfwords, common_mapq):
    """One unit's pair stream -> (entries, switches): entries = [(library, f3, code, mapq pair)] in stream order, switches =
    [(entries in front of it, library it names, 'short' | 'wide')].  Knows the format, not the encoder."""
    entries, switches = [], []
    lib, k, n = 0, 0, len(halfwords)
    while k < n:
        h = int(halfwords[k])
        if h == 0:                                   # no-op: padding
            k += 1
        elif h == WIDE:                              # wide switch: the wide bit alone, then the library
            assert k % 2 == 0 and k + 1 < n, "a wide switch starts on a 4-byte boundary"
            lib = int(halfwords[k + 1])
            switches.append((len(entries), lib, "wide"))
            k += 2
        elif h & WIDE:                               # wide entry: its MAPQ pair follows
            assert k % 2 == 0 and k + 1 < n and (h & 7), "a wide entry starts on a 4-byte boundary and has a straddle bit"
            entries.append((lib, h & 7, (h >> 3) & 0xfff, int(halfwords[k + 1])))
            k += 2
        elif h & 7:                                  # entry with the batch's common MAPQ pair
            entries.append((lib, h & 7, (h >> 3) & 0xfff, common_mapq))
            k += 1
        else:                                        # short switch (l + 1) << 3
            lib = (h >> 3) - 1
            switches.append((len(entries), lib, "short"))
            k += 1
    return entries, switches


def stored_entries(batch, u):
    """what svt_entry_formats.h says unit u's pair stream holds, from the canonical records alone"""
    out = []
    U = batch.units[u]
    is_del, vl, pos_delta = int(U["svtype"]) == 0, int(U["var_length"]), int(U["pos_delta"])
    for r in batch.records[int(batch.rec_offset[u]):int(batch.rec_offset[u + 1])]:
        fl = int(r["flags"])
        L = batch.libs[(fl >> ev.REC_LIB_SHIFT) & 0xffff]
        f3, a, b = fl & 7, int(r["mapq_a"]), int(r["mapq_b"])
        if f3 == 0 or a == 0 or b == 0 or (is_del and float(pos_delta) < 2 * L.sd):
            continue                                 # could only add +0.0: not stored
        nb, x = len(L.hist), int(r["ospan_len"]) - int(L.key_min)
        code = 2 * nb
        if not is_del:
            if 0 <= x < nb:
                code = x
        elif vl < nb:
            if 0 <= x < vl + nb:
                code = x
        elif 0 <= x < nb:
            code = x
        elif 0 <= x - vl < nb:
            code = nb + (x - vl)
        out.append(((fl >> ev.REC_LIB_SHIFT) & 0xffff, f3, code, a | b << 8))
    return out


def _arrays(p):
    return p.slots().tobytes(), p.slot_offset().tobytes(), int(p.c.common_mapq)


def test_257_libraries_pack(fixture_library):
    """the first batch past the old limit: declined as ever without the flag, packed evidence with it"""
    from svtyper_amd import hip
    batch = manylibcases.many_libraries(fixture_library, 257, 3 * 86)
    assert hip.PackedEvidence.try_pack(batch) is None
    p = hip.PackedEvidence.try_pack(batch, many_libraries=True)
    assert p is not None
    with p:
        assert p.c.n_libs == 257 and p.n_units == batch.n_units and p.n_records == batch.n_records
        so = p.slot_offset()
        assert so[0] == 0 and so[-1] == p.c.n_slots and np.all(np.diff(so.astype(np.int64)) >= 0)
        assert p.nbytes < 0.45 * 16 * batch.n_records


@pytest.mark.parametrize("n_libs", [257, 300, 4200])
def test_streams_against_the_records(fixture_library, n_libs):
    """entry for entry: (library, straddle bits, code, MAPQ pair) as the records dictate, a switch exactly where the library
    of the stored entries changes, short below library 256 and wide from there"""
    from svtyper_amd import hip
    batch = manylibcases.many_libraries(fixture_library, n_libs, 6 * ((n_libs + 2) // 3))     # six units per sample
    named, wide_switches, all_switches = set(), 0, 0
    with hip.PackedEvidence(batch, many_libraries=True) as p:
        half = p.slots().view(np.uint16).reshape(-1, 8)
        so, common = p.slot_offset(), int(p.c.common_mapq)
        for u in range(batch.n_units):
            got, switches = decode_pair_stream(half[int(so[3 * u]):int(so[3 * u + 1])].reshape(-1), common)
            want = stored_entries(batch, u)
            assert got == want, u
            # the switches the entries' libraries call for, and no other: the stream starts in library 0
            libs_in_order = [e[0] for e in want]
            expect = [(i, l, "short" if l < SHORT_SWITCH_LIBS else "wide")
                      for i, l in enumerate(libs_in_order) if l != (libs_in_order[i - 1] if i else 0)]
            assert switches == expect, u
            named.update(libs_in_order)
            all_switches += len(switches)
            wide_switches += sum(1 for s in switches if s[2] == "wide")
    assert named == set(range(n_libs)), "every library is named by a stored entry"
    assert wide_switches > 0 and all_switches > wide_switches


@pytest.mark.parametrize("n_libs", [3, 256])
@pytest.mark.parametrize("sso", [0, ev.FLAG_SSO_ASSOCIATION])
def test_slots_of_at_most_256_libraries_did_not_move(fixture_library, n_libs, sso):
    """read by oracle/py_packed.py, which knows the short switch only; the flag changes nothing below the limit"""
    from oracle import c_oracle, py_packed
    from svtyper_amd import hip
    batch = manylibcases.many_libraries(fixture_library, n_libs, 258)
    want = c_oracle.genotype_batch(batch, flags=sso).tallies
    with hip.PackedEvidence(batch) as p, hip.PackedEvidence(batch, many_libraries=True) as q:
        assert _arrays(p) == _arrays(q)
        half = p.slots().view(np.uint16).reshape(-1)
        assert not (half == WIDE).any()
        got = py_packed.tally_packed(p.slots(), p.slot_offset(), batch.units, list(batch.libs), int(p.c.common_mapq), bool(sso))
    skip = (batch.units["flags"] & ev.UNIT_SKIP) != 0
    assert np.array_equal(np.ascontiguousarray(got[~skip]).view(np.uint64), np.ascontiguousarray(want[~skip]).view(np.uint64))


def _with_env(name, value, fn):
    keep = os.environ.get(name)
    os.environ[name] = value
    try:
        return fn()
    finally:
        if keep is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = keep


def test_encoder_forms_write_the_same_slots(fixture_library):
    """300 libraries: sixteen records at a time (AVX-512) and record by record, one worker and several, the ranged encoder; on
    the per-sample batch, on records that alternate across the short / wide boundary, and with continuation records"""
    from svtyper_amd import hip
    per_sample = manylibcases.many_libraries(fixture_library, 300, 2000)
    boundary = manylibcases.interleaved_across_the_boundary(fixture_library)
    cont = manylibcases.interleaved_across_the_boundary(fixture_library, n_units=400)
    firsts = set(int(x) for x in cont.rec_offset[:-1])
    pick = np.array([i for i in range(7, cont.n_records, 31) if i not in firsts])
    cont.records["flags"][pick] = (cont.records["flags"][pick] & 0xffff00) | ev.REC_CONTINUATION
    for name in ("ospan_len", "mapq_a", "mapq_b"):
        cont.records[name][pick] = 0
    no_hint = ev.EvidenceBatch(per_sample.rec_offset, per_sample.units.copy(), per_sample.records, per_sample.libs)
    no_hint.units["libs"] = 0
    for batch in (per_sample, boundary, cont, no_hint):
        def pack():
            with hip.PackedEvidence(batch, many_libraries=True) as p:
                return _arrays(p)
        want = pack()
        assert _with_env("SVT_PACK_SCALAR", "1", pack) == want
        for nt in ("1", "3", "8"):
            assert _with_env("SVT_PACK_THREADS", nt, pack) == want
        for ranges in ("256", "1000"):
            assert _with_env("SVT_PACK_TEST_RANGES", ranges, pack) == want
        assert _with_env("SVT_PACK_SCALAR", "1", lambda: _with_env("SVT_PACK_TEST_RANGES", "512", pack)) == want


def test_limits_that_stay(fixture_library):
    from svtyper_amd import hip
    small = synth.make_units(20, 3, [fixture_library])
    too_many = ev.EvidenceBatch(small.rec_offset, small.units, small.records, [fixture_library] * 65537)
    for many in (False, True):
        with pytest.raises(hip.SvtyperHipError) as e:
            hip.PackedEvidence.try_pack(too_many, many_libraries=many)
        assert "error -1" in str(e.value) and "n_libs must be 1..65536" in str(e.value)
    batch = manylibcases.many_libraries(fixture_library, 300, 2000)
    beyond = ev.EvidenceBatch(batch.rec_offset, batch.units, batch.records.copy(), batch.libs)
    r = int(beyond.rec_offset[1700]) + 1
    for lib in (300, 4094, 65535):
        beyond.records["flags"][r] = (int(beyond.records["flags"][r]) & 0xff) | lib << ev.REC_LIB_SHIFT
        for scalar in (False, True):
            def pack():
                with pytest.raises(hip.SvtyperHipError) as e:
                    hip.PackedEvidence(beyond, many_libraries=True)
                assert "lib index" in str(e.value)
            _with_env("SVT_PACK_SCALAR", "1", pack) if scalar else pack()
    # the other reasons to keep the canonical records are what they were
    wide_hist = ev.EvidenceBatch(batch.rec_offset, batch.units, batch.records, list(batch.libs[:299]) + [synth.normal_library(3000.0, 900.0, seed=5)])
    assert hip.PackedEvidence.try_pack(wide_hist, many_libraries=True) is None
    neg = ev.EvidenceBatch(batch.rec_offset, batch.units.copy(), batch.records, batch.libs)
    d = int(np.nonzero(neg.units["svtype"] == 0)[0][0])
    neg.units["var_length"][d] = -7
    assert hip.PackedEvidence.try_pack(neg, many_libraries=True) is None

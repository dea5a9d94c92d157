"""GPU: the geometry kernel (svt_geometry_kernel) and the device reader against tests/golden/geometry_edges.json.gz, the boundary
lattice whose records, tallies and results the REFERENCE made (tests/geomcases.py; its reach is asserted on the CPU by
tests/test_geometry_edges.py), and the kernel's unit look-up around empty units."""
import numpy as np
import pytest

import fakereads
import geomcases as G
import goldenio as gio
from svtyper_amd import evidence as ev
from svtyper_amd import fragments as fr
from svtyper_amd import geometry as geo
from svtyper_amd import native_reads as nr
from svtyper_amd import packer
from svtyper_amd.results import result_from_record
from test_geometry_edges import assert_records_equal, golden_unit_records
from test_hip_geometry import _Lib, _fragment_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return gio.load("geometry_edges.json.gz")


def test_kernel_gives_the_reference_records_and_results(hip_device, golden):
    from svtyper_amd import hip
    n_rec = 0
    for grp in golden["groups"]:
        # (a fragment summary carries 32-bit coordinates: the pair that ends beyond 2^31 - 1 stays with the Python reader)
        grp = dict(grp, sites=[s for s in grp["sites"] if s["fits_int32"]])
        fb = _fragment_batch(grp)
        off, want = golden_unit_records(grp)
        assert np.array_equal(fb.frag_offset, off)
        with hip.DeviceBatch.from_fragments(fb, hip_device, ev.FLAG_SSO_ASSOCIATION, return_records=True) as d:
            assert_records_equal(d.records, want, grp["name"])
            n_rec += len(want)
            d.genotype()
            got = d.results()
            for k, s in enumerate(grp["sites"]):
                gio.assert_result_equal(result_from_record(got.rec[k]), gio.golden_result(s["result"]), 1e-6, s["breakpoint"]["id"])
                if not s["reads"]:       # an empty unit: the blank result, in its place
                    assert result_from_record(got.rec[k])["formats"]["GT"] == "./." and off[k] == off[k + 1]
    assert n_rec > 3000


# units of the look-up test: 257 fragments, so that fragments 255 and 256 lie on both sides of a block of 256 next to empty units
LAYOUT = [0, 0, 0, 1, 0, 0, 254, 0, 1, 1, 0, 0, 0, 0]
POS_A = G.LOOKUP_POS_A


def test_unit_lookup_with_empty_units(hip_device):
    """every record is geometry_record for the breakpoint of the unit that OWNS the fragment: leading, trailing and consecutive
    empty units around a block boundary; neighbouring units differ in pos_a so that a wrong unit gives another record.  The
    expectation comes from the Python predicates (fragments.py + packer.py), not from a second device call."""
    from svtyper_amd import hip
    assert sum(LAYOUT) == 257 and len(LAYOUT) == 14
    spec = G.library_specs()[0]
    lib = _Lib(spec[0], spec[2], spec[3])
    table = ev.LibraryTable.from_counter(spec[5], spec[2], spec[3], spec[0])
    lib_index = {id(lib): 0}
    tid_of = lambda c: {"1": 0, "2": 1}.get(c, -1)
    b = geo.FragmentBatchBuilder([table], 1.0, 1.0, 20, 3)
    want, seen = [], set()
    for u, n in enumerate(LAYOUT):
        bp = {"id": "u%d" % u, "svtype": "DEL", "var_length": 4000,
              "A": {"chrom": "1", "pos": POS_A[u % len(POS_A)], "ci": [0, 0], "is_reverse": False},
              "B": {"chrom": "1", "pos": 5000, "ci": [0, 0], "is_reverse": True}}
        frags = {}
        for k in range(n):
            name = "u%02d.f%03d" % (u, k)
            frags[name] = fr.SamFragment(fakereads.FakeRead(name, 97, "1", 1000, "101M", 60, rg="rg0"), lib)
            frags[name].add_read(fakereads.FakeRead(name, 145, "1", 1300, "101M", 37, rg="rg0"))
        b.add(geo.breakpoint_record(bp, tid_of), geo.summarise_fragments(frags, bp, lib_index, tid_of))
        rec = packer.pack_fragments(frags, bp, lib_index, 20, 3)
        want.append(rec)
        if n:
            seen.add(rec[0].tobytes())
    assert len(seen) >= 3          # the units that own fragments show different records
    fb = b.build()
    assert fb.n_fragments == 257 and fb.n_units == 14
    want = np.concatenate(want)
    with hip.DeviceBatch.from_fragments(fb, hip_device, ev.FLAG_SSO_ASSOCIATION, return_records=True) as d:
        assert_records_equal(d.records, want, "unit look-up")


@pytest.mark.parametrize("inflate", ["host", "device"])
def test_device_reader_gives_the_reference_records(hip_device, golden, tmp_path, inflate):
    import walkcases as W
    for grp in golden["groups"]:
        if not grp["bam"]:
            continue
        sites, sample, nbam = G.write_group_bam(tmp_path, grp, grp["libraries"])
        off, want = golden_unit_records(grp)
        a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
        head = W.header_batch(sample, a[1])
        d, skipped, stats = nbam.evidence_device(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, head, hip_device,
                                                 ev.FLAG_SSO_ASSOCIATION, 2, inflate=inflate)
        try:
            got_off, recs = nr.batch_records(d)
            assert stats["units_host"] == 0, stats["units_host_by_reason"]
            assert not skipped.any() and np.array_equal(got_off, off)
            assert_records_equal(recs, want, "device reader, inflate=%s" % inflate)
            d.genotype()
            got = d.results()
            for k, s in enumerate(grp["sites"]):
                gio.assert_result_equal(result_from_record(got.rec[k]), gio.golden_result(s["result"]), 1e-6, s["breakpoint"]["id"])
        finally:
            d.close()

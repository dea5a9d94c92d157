"""The C-ABI library loads and exports every symbol include/svtyper_hip.h declares (no compute:
runs without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header="svtyper_hip.h"):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(svt_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported():
    from svtyper_amd import hip
    hip.build()
    lib = ctypes.CDLL(hip.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(lib, s), "missing export %s" % s
    assert sorted(hip.EXPORTS) == syms
    reads = declared_symbols("svtyper_reads.h")
    assert len(reads) >= 9
    for s in reads:
        assert hasattr(lib, s), "missing export %s" % s


def test_version_and_loud_failure_without_gpu():
    from svtyper_amd import hip, synth
    L = hip.load()
    assert L.svt_version() == hip.ABI_VERSION
    if hip.device_count() == 0:
        import pytest
        b = synth.make_units(10, 1, [synth.normal_library(n=20000)])
        with pytest.raises(hip.SvtyperHipError) as e:
            hip.genotype_batch(b)
        assert "no CPU fallback" in str(e.value) or "no HIP device" in str(e.value)


def test_native_sample_column_text_equals_python_formatting():
    """svt_format_results (host-only) == results.results_to_dicts + vcf.Genotype.get_gt_string, for every GT
    code, both skip conventions and several FORMAT orders (including keys the sample has no value for)."""
    import numpy as np
    from svtyper_amd import evidence as ev, hip, synth
    from svtyper_amd.results import results_to_dicts
    from oracle import c_oracle
    lib = synth.normal_library(n=30000)
    res = c_oracle.genotype_batch(synth.make_edge_cases([lib], seed=3), 0)
    codes = set(np.unique(res.gt).tolist())
    assert {ev.GT_BLANK, ev.GT_SKIPPED, ev.GT_MISSING, 0, 1, 2} <= codes
    ours = ("GT", "GQ", "SQ", "GL", "DP", "RO", "AO", "QR", "QA", "RS", "AS", "ASC", "RP", "AP", "AB")
    orders = [ours, ("GT", "SU", "GQ", "DP", "CN", "SQ", "GL", "RO", "AO", "QR", "QA", "RS", "AS", "ASC", "RP", "AP", "AB"),
              ("GT",), ("AB", "GL", "GT")]
    dicts = results_to_dicts(res)
    gts = res.gt.tolist()

    def cell(v):
        return "%0.2f" % v if type(v) == float else str(v)

    for fields in orders:
        for skipped_as_dots in (False, True):
            got = hip.format_results(res, fields, skipped_as_dots)
            assert len(got) == res.n_units
            for i, (d, gt) in enumerate(zip(dicts, gts)):
                if gt == ev.GT_SKIPPED and skipped_as_dots:       # classic.py:282-284: only GT is set
                    want = ":".join("./." if f == "GT" else "." for f in fields)
                else:
                    want = ":".join(cell(d["formats"][f]) if f in d["formats"] else "." for f in fields)
                assert got[i] == want, (i, gt, fields, got[i], want)


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of every struct of include/svtyper_hip.h, as a C compiler lays them out, against the numpy
    dtypes and ctypes Structures the Python side hands to the library (and the INTEGRATION.md stub copies)."""
    import subprocess
    import numpy as np
    from svtyper_amd import evidence as ev, geometry as geo
    structs = {
        "svt_record": ["ospan_len", "mapq_a", "mapq_b", "rs_a", "rs_b", "seq_l", "seq_r", "clip_l", "clip_r", "flags"],
        "svt_unit": ["var_length", "pos_delta", "sample", "svtype", "flags", "libs"],
        "svt_library": ["hist", "key_min", "n_bins", "mean", "sd"],
        "svt_evidence_batch": ["n_units", "rec_offset", "units", "records", "n_libs", "libs", "split_weight", "disc_weight"],
        "svt_read_summary": ["tid", "start", "end", "iv_start", "iv_end", "mapq", "flags", "reserved"],
        "svt_piece_summary": ["tid", "start", "end", "mapq", "flags", "reserved"],
        "svt_fragment": ["read", "seq", "clip"],
        "svt_breakpoint": ["tid_a", "pos_a", "ci_a", "tid_b", "pos_b", "ci_b", "var_length", "sample", "svtype", "flags", "reserved"],
        "svt_fragment_batch": ["n_units", "frag_offset", "breakpoints", "fragments", "n_libs", "libs", "split_weight",
                               "disc_weight", "min_aligned", "split_slop"],
        "svt_result": ["gl", "sq", "tallies", "counts", "gt", "pad"],
        "svt_result96": ["gl", "sq", "tallies", "qr", "qa", "gq", "gt", "pad", "unit", "pad2"],
    }
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "svtyper_hip.h"', 'int main(void) {']
    for name, fields in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    for macro in ("SVT_ABI_VERSION", "SVT_FLAG_SSO_ASSOCIATION", "SVT_FLAG_GENERAL_TABLES", "SVT_FLAG_RESULT96", "SVT_NO_UNIT", "SVT_REC_LIB_SHIFT", "SVT_REC_CONTINUATION", "SVT_REC_HAS_PAIR"):
        lines.append('printf("%s %%d\\n", (int)%s);' % (macro, macro))
    lines += ['return 0; }']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    c = dict(l.split() for l in subprocess.check_output([exe], text=True).splitlines())
    c = {k: int(v) for k, v in c.items()}

    from svtyper_amd import hip
    assert c["SVT_ABI_VERSION"] == hip.ABI_VERSION
    assert (c["SVT_FLAG_SSO_ASSOCIATION"], c["SVT_FLAG_GENERAL_TABLES"]) == (ev.FLAG_SSO_ASSOCIATION, ev.FLAG_GENERAL_TABLES)
    assert (c["SVT_REC_LIB_SHIFT"], c["SVT_REC_CONTINUATION"], c["SVT_REC_HAS_PAIR"]) == (ev.REC_LIB_SHIFT, ev.REC_CONTINUATION, ev.REC_HAS_PAIR)
    assert c["SVT_FLAG_RESULT96"] == ev.FLAG_RESULT96 and c["svt_result96"] == 96
    # the 96-byte record is svt_result's first 84 bytes + gt: what svt_results_expand96 and the kernel's store rely on
    assert c["svt_result96.qr"] == c["svt_result.counts"] == 72 and c["svt_result96.gt"] == 84 and c["svt_result.gt"] == 116
    assert c["svt_result96.unit"] == 88 and c["SVT_NO_UNIT"] == ev.NO_UNIT - (1 << 32)
    dtypes = {"svt_record": ev.RECORD_DTYPE, "svt_unit": ev.UNIT_DTYPE, "svt_result": ev.RESULT_DTYPE, "svt_result96": ev.RESULT96_DTYPE,
              "svt_read_summary": geo.READ_DTYPE, "svt_piece_summary": geo.PIECE_DTYPE, "svt_fragment": geo.FRAGMENT_DTYPE,
              "svt_breakpoint": geo.BREAKPOINT_DTYPE}
    for name, dt in dtypes.items():
        assert dt.itemsize == c[name], (name, dt.itemsize, c[name])
        assert list(dt.names) == structs[name], (name, dt.names)
        for f in dt.names:
            assert dt.fields[f][1] == c["%s.%s" % (name, f)], (name, f, dt.fields[f][1], c["%s.%s" % (name, f)])
    assert c["svt_record"] == 16 and c["svt_unit"] == 16 and c["svt_result"] == 128 and c["svt_fragment"] == 128
    ctys = {"svt_library": ev.CLibrary, "svt_evidence_batch": ev.CEvidenceBatch, "svt_fragment_batch": geo.CFragmentBatch}
    for name, ct in ctys.items():
        assert ctypes.sizeof(ct) == c[name], (name, ctypes.sizeof(ct), c[name])
        assert [f[0] for f in ct._fields_] == structs[name], name
        for f in structs[name]:
            assert getattr(ct, f).offset == c["%s.%s" % (name, f)], (name, f)
    # the enumerations the result record is indexed with
    assert list(ev.COUNT_NAMES) == ["QR", "QA", "GQ", "DP", "RO", "AO", "RS", "AS", "ASC", "RP", "AP"]
    assert list(ev.TALLY_NAMES) == ["ref_seq", "alt_seq", "alt_clip", "ref_span", "alt_span"]


def _evidence(n_units=2, n_records=4, n_libs=1, libs=True, records=True, rec_offset0=0, split_weight=1.0, disc_weight=1.0):
    """A small svt_evidence_batch (ctypes) and the arrays it points at (keep them alive while it is used)."""
    import numpy as np
    from svtyper_amd import evidence as ev
    off = np.linspace(0, n_records, n_units + 1).astype(np.uint64)
    off[0] = rec_offset0
    units = np.zeros(n_units, ev.UNIT_DTYPE)
    recs = np.zeros(max(n_records, 1), ev.RECORD_DTYPE)
    hist = np.ones(4, np.uint32)
    clibs = (ev.CLibrary * max(n_libs, 1))()
    for l in clibs:
        l.hist = hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        l.n_bins, l.mean, l.sd = 4, 300.0, 30.0
    cb = ev.CEvidenceBatch()
    cb.n_units = n_units
    cb.rec_offset = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    cb.units = units.ctypes.data
    cb.records = recs.ctypes.data if records else None
    cb.n_libs = n_libs
    cb.libs = clibs if libs else None
    cb.split_weight, cb.disc_weight = split_weight, disc_weight
    return cb, (off, units, recs, hist, clibs)


def _fragments(n_units=2, n_frags=4, n_libs=1, frag_offset0=0, fragments=True):
    import numpy as np
    from svtyper_amd import evidence as ev, geometry as geo
    off = np.linspace(0, n_frags, n_units + 1).astype(np.uint64)
    off[0] = frag_offset0
    bps = np.zeros(n_units, geo.BREAKPOINT_DTYPE)
    frags = np.zeros(max(n_frags, 1), geo.FRAGMENT_DTYPE)
    hist = np.ones(4, np.uint32)
    clibs = (ev.CLibrary * max(n_libs, 1))()
    for l in clibs:
        l.hist = hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        l.n_bins, l.mean, l.sd = 4, 300.0, 30.0
    fb = geo.CFragmentBatch()
    fb.n_units = n_units
    fb.frag_offset = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    fb.breakpoints = bps.ctypes.data
    fb.fragments = frags.ctypes.data if fragments else None
    fb.n_libs = n_libs
    fb.libs = clibs
    fb.split_weight = fb.disc_weight = 1.0
    fb.min_aligned, fb.split_slop = 20, 7
    return fb, (off, bps, frags, hist, clibs)


def test_entry_point_argument_errors():
    """Inputs the C entry points refuse before they touch a device: the return code and the exact svt_last_error()
    text, including which check fires first when several would."""
    import numpy as np
    from svtyper_amd import evidence as ev, hip
    L = hip.load()
    nan = float("nan")
    INVALID, NO_DEVICE = -1, -2
    out = np.zeros(64, ev.RESULT_DTYPE)
    h = ctypes.c_void_p()

    def create(**kw):
        flags = kw.pop("flags", 0)
        cb, keep = _evidence(**kw)
        return L.svt_batch_create(ctypes.byref(cb), 0, flags, ctypes.byref(h))

    def segments(n_segments=1, seg_records=4, flags=0, **kw):
        cb, keep = _evidence(records=False, **kw)
        recs = np.zeros(max(seg_records, 1), np.dtype([("x", "u1", 16)]))
        segs = np.zeros(max(n_segments, 1), np.dtype([("records", "<u8"), ("n_records", "<u8")]))
        for k in range(n_segments):
            segs[k] = (recs.ctypes.data, seg_records // n_segments)
        return L.svt_batch_create_segments(ctypes.byref(cb), segs.ctypes.data, n_segments, 0, flags, ctypes.byref(h))

    def fragments(flags=0, **kw):
        fb, keep = _fragments(**kw)
        return L.svt_batch_create_from_fragments(ctypes.addressof(fb), 0, flags, None, ctypes.byref(h))

    def genotype(flags=0, **kw):
        cb, keep = _evidence(**kw)
        return L.svt_genotype(ctypes.byref(cb), out.ctypes.data, 0, flags)

    def multi(devices=(0,), n_devices=None, flags=0, monotone=True, **kw):
        cb, keep = _evidence(**kw)
        if not monotone:
            keep[0][1] = 3
            keep[0][2] = 1
        devs = (ctypes.c_int * max(len(devices), 1))(*devices)
        n = len(devices) if n_devices is None else n_devices
        return L.svt_genotype_multi(ctypes.byref(cb), out.ctypes.data, devs, n, 1, flags)

    def packed_from_records(flags=0, **kw):
        cb, keep = _evidence(**kw)
        return L.svt_genotype_packed_from_records(ctypes.byref(cb), out.ctypes.data, 0, flags)

    n_libs_text = "n_libs must be 1..65536"
    weights_text = "weights must be finite and >= 0"
    cases = [
        # svt_batch_create
        ("create null", lambda: L.svt_batch_create(None, 0, 0, ctypes.byref(h)), INVALID, "null argument"),
        ("create null out", lambda: L.svt_batch_create(ctypes.byref(_evidence()[0]), 0, 0, None), INVALID, "null argument"),
        ("create flags", lambda: create(flags=1 << 20), INVALID, "unknown flag bits"),
        ("create flags first", lambda: create(flags=1 << 20, n_libs=0, split_weight=nan), INVALID, "unknown flag bits"),
        ("create n_libs 0", lambda: create(n_libs=0), INVALID, n_libs_text),
        ("create n_libs 65537", lambda: create(n_libs=65537), INVALID, n_libs_text),
        ("create libs null", lambda: create(libs=False), INVALID, n_libs_text),
        ("create n_libs before offsets", lambda: create(n_libs=0, rec_offset0=1), INVALID, n_libs_text),
        ("create rec_offset[0]", lambda: create(rec_offset0=1), INVALID, "rec_offset[0] must be 0"),
        ("create offsets before records", lambda: create(rec_offset0=1, records=False), INVALID, "rec_offset[0] must be 0"),
        ("create null records", lambda: create(records=False), INVALID, "null records"),
        ("create records before weights", lambda: create(records=False, disc_weight=nan), INVALID, "null records"),
        ("create NaN weight", lambda: create(split_weight=nan), INVALID, weights_text),
        ("create negative weight", lambda: create(disc_weight=-1.0), INVALID, weights_text),
        ("create infinite weight", lambda: create(split_weight=float("inf")), INVALID, weights_text),
        # svt_batch_create_segments (the records come in the segments: a null `records` is not an error)
        ("segments null", lambda: L.svt_batch_create_segments(None, None, 0, 0, 0, ctypes.byref(h)), INVALID, "null argument"),
        ("segments null list", lambda: L.svt_batch_create_segments(ctypes.byref(_evidence()[0]), None, 1, 0, 0, ctypes.byref(h)),
         INVALID, "null argument"),
        ("segments fewer", lambda: segments(seg_records=2), INVALID,
         "svt_batch_create_segments: the segments hold fewer records than rec_offset[n_units]"),
        ("segments more", lambda: segments(n_segments=2, seg_records=8), INVALID,
         "svt_batch_create_segments: the segments hold more records than rec_offset[n_units]"),
        ("segments flags", lambda: segments(flags=1 << 20, n_records=0, seg_records=0, n_segments=0), INVALID, "unknown flag bits"),
        ("segments n_libs 0", lambda: segments(n_libs=0), INVALID, n_libs_text),
        ("segments rec_offset[0]", lambda: segments(rec_offset0=1), INVALID, "rec_offset[0] must be 0"),
        ("segments NaN weight", lambda: segments(split_weight=nan), INVALID, weights_text),
        ("segments negative weight", lambda: segments(disc_weight=-0.5), INVALID, weights_text),
        # svt_batch_create_from_fragments
        ("fragments null", lambda: L.svt_batch_create_from_fragments(None, 0, 0, None, ctypes.byref(h)), INVALID, "null argument"),
        ("fragments flags", lambda: fragments(flags=1 << 20), INVALID, "unknown flag bits"),
        ("fragments n_libs 0", lambda: fragments(n_libs=0), INVALID, n_libs_text),
        ("fragments n_libs 65537", lambda: fragments(n_libs=65537), INVALID, n_libs_text),
        ("fragments frag_offset[0]", lambda: fragments(frag_offset0=1), INVALID, "frag_offset[0] must be 0"),
        ("fragments null fragments", lambda: fragments(fragments=False), INVALID, "null fragments"),
        # svt_genotype
        ("genotype null", lambda: L.svt_genotype(None, out.ctypes.data, 0, 0), INVALID, "null argument"),
        ("genotype flags", lambda: genotype(flags=1 << 20), INVALID, "unknown flag bits"),
        ("genotype n_libs 0", lambda: genotype(n_libs=0), INVALID, n_libs_text),
        ("genotype n_libs 65537", lambda: genotype(n_libs=65537), INVALID, n_libs_text),
        ("genotype rec_offset[0]", lambda: genotype(rec_offset0=1), INVALID, "rec_offset[0] must be 0"),
        ("genotype null records", lambda: genotype(records=False), INVALID, "null records"),
        ("genotype NaN weight", lambda: genotype(split_weight=nan), INVALID, weights_text),
        ("genotype negative weight", lambda: genotype(disc_weight=-1.0), INVALID, weights_text),
        # svt_genotype_multi (the device list is checked before the offsets' monotony)
        ("multi null", lambda: L.svt_genotype_multi(None, out.ctypes.data, (ctypes.c_int * 1)(0), 1, 1, 0), INVALID, "bad device list"),
        ("multi null devices", lambda: L.svt_genotype_multi(ctypes.byref(_evidence()[0]), out.ctypes.data, None, 1, 1, 0),
         INVALID, "bad device list"),
        ("multi no devices", lambda: multi(n_devices=0), INVALID, "bad device list"),
        ("multi 65 devices", lambda: multi(devices=(0,) * 65), INVALID, "bad device list"),
        ("multi null out", lambda: L.svt_genotype_multi(ctypes.byref(_evidence()[0]), None, (ctypes.c_int * 1)(0), 1, 1, 0),
         INVALID, "null argument"),
        ("multi device -1", lambda: multi(devices=(0, -1), monotone=False), NO_DEVICE,
         "device index out of range" if hip.device_count() > 0 else "no HIP device available (this library has no CPU fallback)"),
        # svt_genotype_packed_from_records
        ("packed null", lambda: L.svt_genotype_packed_from_records(None, out.ctypes.data, 0, 0), INVALID, "null argument"),
        ("packed null out", lambda: L.svt_genotype_packed_from_records(ctypes.byref(_evidence()[0]), None, 0, 0), INVALID,
         "null argument"),
        ("packed flags", lambda: packed_from_records(flags=1 << 20), INVALID,
         "packed evidence takes SVT_FLAG_SSO_ASSOCIATION and SVT_FLAG_RESULT96 only"),
        ("packed general tables", lambda: packed_from_records(flags=ev.FLAG_GENERAL_TABLES), INVALID,
         "packed evidence takes SVT_FLAG_SSO_ASSOCIATION and SVT_FLAG_RESULT96 only"),
        ("packed n_libs 0", lambda: packed_from_records(n_libs=0), INVALID, n_libs_text),
    ]
    for name, call, code, text in cases:
        got = call()
        assert (got, L.svt_last_error().decode()) == (code, text), name


def test_only_the_c_abi_is_exported():
    """Every dynamic symbol the library defines is a svt_* C entry point (svt_exports.map): its C++ internals can be
    neither interposed on nor reached from outside."""
    import subprocess
    from svtyper_amd import hip
    hip.build()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", hip.LIB_PATH], text=True)
    names = [l.split()[-1] for l in nm.splitlines() if l.strip()]
    assert len(names) >= len(declared_symbols()) + len(declared_symbols("svtyper_reads.h"))
    assert [n for n in names if not n.startswith("svt_")] == []

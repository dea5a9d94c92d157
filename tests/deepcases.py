"""Inputs shared by tests/test_deep_units_host.py (CPU) and tests/test_deep_units_device.py (GPU): units of more kept reads than
the on-chip tier of the evidence walk holds (walk_capacities()["reads_lds"] = 1 024), up to and beyond the deep tier's 16 384.
The reference of every comparison is the host reader, svt_bam_evidence (NativeBam.evidence)."""
import numpy as np

import walkcases as W
from svtyper_amd import native_reads as nr

LDS, DEEP = 1024, 16384                                 # the two capacities (test_capacities pins them to the library's)
BOUNDARIES = (1024, 1025, 4097, 16384)                  # kept reads of the one unit of boundary_input: inside the envelope
OVER = 16385                                            # ... and the first count outside it
BAND_LOW, BAND_HIGH = (1025, 4096), (8192, 16384)

# name -> (seed, n_pairs, arguments of the generator, the band its one covered unit has to land in)
REALISTIC = {
    "low": (5, 1500, {}, BAND_LOW),
    "low_tied": (6, 1500, {"tied_names": True}, BAND_LOW),
    "low_sa_first": (7, 1500, {"sa_first": True}, BAND_LOW),
    "high": (5, 6000, {}, BAND_HIGH),
    "high_tied": (6, 6000, {"tied_names": True}, BAND_HIGH),
    "high_sa_first": (7, 6000, {"sa_first": True}, BAND_HIGH),
}
# (count mode, max_reads): both modes without a limit, a limit that skips the unit and one that keeps it, in both modes
MODES = ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, None), (nr.COUNT_SSO, 1000), (nr.COUNT_CLASSIC, 1000), (nr.COUNT_SSO, 100000),
         (nr.COUNT_CLASSIC, 100000))


def realistic_input(tmp_path, name):
    seed, n_pairs, kw, band = REALISTIC[name]
    return W.synthetic_input(tmp_path, seed, n_pairs=n_pairs, only_sites=[0], **kw) + (band,)


def host_reader(sites, sample, nbam, mode, max_reads, threads=2):
    """(unit arrays, (rec_offset, records, skipped) of svt_bam_evidence)"""
    a = W.unit_arrays(sites, sample, nbam, mode)
    return a, nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, threads)


def walk(nbam, a, mode, max_reads, entry, threads=2):
    return getattr(nbam, entry)(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, threads)


def assert_units_equal(want, off, recs, skipped, units=None):
    """rec_offset / records / skipped of `units` (default: all) byte for byte; `off` may come from a result whose other units
    are empty (the walk without a fallback), so records are compared unit by unit"""
    n = len(want[0]) - 1
    for u in (range(n) if units is None else units):
        assert int(skipped[u]) == int(want[2][u]), "unit %d: skip flag" % u
        w = want[1][int(want[0][u]):int(want[0][u + 1])]
        g = recs[int(off[u]):int(off[u + 1])]
        assert len(g) == len(w), "unit %d: %d records, the host reader has %d" % (u, len(g), len(w))
        assert g.tobytes() == w.tobytes(), "unit %d: records differ" % u


def _margin_site(a, ident):
    return {"breakpoint": {"id": ident, "svtype": "DEL", "var_length": 400, "A": {"chrom": "1", "pos": a, "ci": [0, 0], "is_reverse": False},
                           "B": {"chrom": "1", "pos": a + 401, "ci": [0, 0], "is_reverse": True}}}


def mixed_input(tmp_path):
    """One call with over-deep, deep, shallow and empty units: 40 000 pairs over the generator's sites 0 and 3 (about 47 k and
    40 k kept reads), its sites 1 and 2 without a read, and four more sites on the thinning left margin of site 0's reads
    (measured: 521, 2 148, 6 166 and 9 632 kept reads).  The tests take the tiers from kept_reads, not from these figures."""
    sites, sample, nbam = W.synthetic_input(tmp_path, 5, n_pairs=40000, only_sites=[0, 3])
    return sites + [_margin_site(a, "m%d" % a) for a in (48_700, 48_800, 49_000, 49_100)], sample, nbam


def tiers(kept):
    """(shallow, deep, over-deep) unit indices by kept reads"""
    kept = np.asarray(kept)
    return (np.flatnonzero(kept <= LDS).tolist(), np.flatnonzero((kept > LDS) & (kept <= DEEP)).tolist(),
            np.flatnonzero(kept > DEEP).tolist())


# ---- hand-built names (walkcases.HEADER / SITE / INFO: one library, one window pair around 50 050 / 50 851) ----------------------
def _pos(k):
    return 50_000 + k % 60


def adversarial_cases():
    """name -> records of one deep unit whose order hangs on what the 8-byte key cannot see"""
    rg = ("RG", "Z", "rg")
    split = dict(cigar="60M40S", tags=[rg, ("SA", "Z", "1,50801,+,60S40M,60,0;")])
    # names that are prefixes of one another: "p", "pp", ... up to the cap, each several times, in an order that is not sorted
    prefixes = [W._read("p" * (1 + (7 * k) % 128), _pos(k), flag=(0x1 | 0x40) if k % 2 else (0x1 | 0x80)) for k in range(1500)]
    # the first byte varies over the reads, so the unit has no common prefix and the key is a name's first eight bytes; behind
    # the first byte come seven (or more) bytes every name shares, and the names of one first byte differ only behind byte 8, some
    # in the next byte and some sixteen bytes further back: the order of each group hangs on whole-name compares alone
    behind = [W._read("abc"[k % 3] + "/lane07" + ("" if k % 5 else "/tile0000/x0y0z0") + "%04d" % ((k * 37) % 900), _pos(k),
                      flag=(0x1 | 0x40) if k % 3 else (0x1 | 0x80), **(split if k % 11 == 0 else {})) for k in range(1800)]
    # one name 3 000 times with alternating flags (the repeated (name, flag) is dropped along a long run), among other reads
    one_name = [W._read("same", _pos(k), flag=0x1 | (0x40 if k % 2 == 0 else 0x80) | (0x10 if k % 4 == 1 else 0) | (0x100 if k % 50 == 7 else 0),
                        **(split if k == 3 else {})) for k in range(3000)]
    one_name += [W._read("o%03d" % (k % 150), _pos(k), flag=(0x1 | 0x40) if k % 2 else (0x1 | 0x80)) for k in range(300)]
    # names at the 128-byte cap, and pairs of them, under two first bytes: no common prefix, two keys in the whole unit, and
    # every compare between names of one first byte runs 122 bytes deep before it meets the difference
    capped = [W._read("nm"[k % 2] + "n" * 121 + "%06d" % ((k * 7919) % 700), _pos(k), flag=(0x1 | 0x40) if k % 4 < 2 else (0x1 | 0x80),
                      **(split if k % 13 == 0 else {})) for k in range(1400)]
    return {"prefixes": prefixes, "behind_the_key": behind, "one_name": one_name, "name_cap": capped}


def names_behind_equal_keys(records):
    """How many different names of `records` share their walk key with another name.  The key is the walk's (walk_unit in
    svt_evidence_walk.h): the eight bytes behind the common prefix of all names, zeros behind a name's end.  It is the unit's
    key when the unit keeps every record, which the caller checks."""
    names = sorted({r["name"].encode() for r in records})
    lcp = 0
    while all(len(n) > lcp and n[lcp] == names[0][lcp] for n in names):
        lcp += 1
    by_key = {}
    for n in names:
        by_key.setdefault(n[lcp:lcp + 8].ljust(8, b"\0"), []).append(n)
    return sum(len(g) for g in by_key.values() if len(g) > 1)


# the cases that are there for the compare behind the key, and their number of different names (k and k + 900, or k + 700, give
# one name): every one of them shares its key with others -- three keys over 900 names, two keys over 700
EQUAL_KEY_NAMES = {"behind_the_key": 900, "name_cap": 700}


def adversarial_input(tmp_path, case):
    sample, nbam = W.open_sample(W.write_case(tmp_path, "adv_" + case, adversarial_cases()[case]), W.INFO)
    return [{"breakpoint": W.SITE}], sample, nbam


def many_deep_input(tmp_path, n_sites, reads_per_site=1100):
    """`n_sites` deep units of `reads_per_site` kept reads each: more of them than the deep workspace has slices"""
    import bamwriter as bw
    length = 2000 * n_sites + 100_000
    header = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:%d\n@RG\tID:rg\tSM:s\tLB:lib\n" % length
    records, sites = [], []
    for s in range(n_sites):
        at = 10_000 + 2000 * s                          # windows of +- 500 around `at` and `at + 801`: the sites do not share reads
        sites.append({"breakpoint": {"id": "s%d" % s, "svtype": "DEL", "var_length": 800,
                                     "A": {"chrom": "1", "pos": at + 50, "ci": [0, 0], "is_reverse": False},
                                     "B": {"chrom": "1", "pos": at + 851, "ci": [0, 0], "is_reverse": True}}})
        for k in range(reads_per_site):
            r = W._read("s%dq%04d" % (s, (k * 13) % (reads_per_site // 2 + 50)), at + k % 40,
                        flag=0x1 | (0x40 if k % 2 else 0x80) | (0x10 if k % 5 == 0 else 0))
            r["mpos"] = at + 300
            records.append(r)
    path = str(tmp_path / ("many%d.bam" % n_sites))
    bw.write_bam(path, header, [("1", length)], sorted(records, key=lambda r: r["pos"]))
    sample, nbam = W.open_sample(path, W.INFO)
    return sites, sample, nbam


def driver_case(tmp_path, n_pairs=6000):
    """(bam, vcf, library json) for the drivers: the generator's four sites at a depth of about 3 500 kept reads per unit
    (every unit is a deep one), and a VCF with those sites (the lines of test_multisample_qual.three_sample_case)"""
    import json
    import test_host_pipeline as H
    import test_native_reads as N
    bam = str(tmp_path / "deep.bam")
    _sites, info = N._synthetic_bam(bam, seed=81, n_pairs=n_pairs, sample="deep")
    lib_json = str(tmp_path / "deep.json")
    with open(lib_json, "w") as f:
        json.dump(info, f)
    header = [l for l in open(H.IN_VCF) if l.startswith("##")]
    body = [
        "1\t50000\td1\tN\t<DEL>\t12.5\t.\tSVTYPE=DEL;SVLEN=-800;END=50800;STR=+-:10;CIPOS=-5,5;CIEND=-5,5\n",
        "1\t90000\tu1\tN\t<DUP>\t7\t.\tSVTYPE=DUP;SVLEN=1500;END=91500;STR=-+:10;CIPOS=0,0;CIEND=0,0\n",
        "1\t120000\ti1\tN\t<INV>\t0\t.\tSVTYPE=INV;SVLEN=3000;END=123000;STR=++:5,--:5;CIPOS=-10,10;CIEND=-10,10\n",
        "1\t150000\tb1_1\tN\tN]2:40000]\t3.25\t.\tSVTYPE=BND;STR=++:7;CIPOS=-2,2;CIEND=-2,2;MATEID=b1_2;EVENT=b1\n",
        "2\t40000\tb1_2\tN\tN]1:150000]\t3.25\t.\tSVTYPE=BND;STR=++:7;CIPOS=-2,2;CIEND=-2,2;MATEID=b1_1;EVENT=b1;SECONDARY\n",
    ]
    vcf = str(tmp_path / "deep.vcf")
    with open(vcf, "w") as f:
        f.write("".join(header) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(body))
    return bam, vcf, lib_json

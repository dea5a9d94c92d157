"""Boundary lattice for the breakpoint-dependent geometry predicates (TEST INFRASTRUCTURE).

Two things live here, both independent of svtyper_amd/csrc/svt_geometry_math.h:

* `census(...)`: a plain restatement of the reference's predicates (svtyper/parsers.py:785-857 `get_ispan`, `is_ref_seq`,
  `is_pair_straddle`; :1122-1215 `check_split_support`, `is_split_straddle`), written from the reference's text.  For one
  (breakpoint, reads, libraries) site it gives, per fragment in `sorted(query_name)` order, the verdict of every predicate and
  the list of boundary EVENTS the fragment sits on: (predicate, side, orientation, signed distance to the threshold, ...).
  Which split candidates exist is restated by shape only (SA tag with one entry; soft clip without SA): the candidate QC of
  SplitRead.is_valid (non-overlap, off-diagonal distance, desert) is not restated, the reach test checks the verdicts against
  the reference's records instead.
* `corpus()`: a deterministic generator of FakeRead sites that puts fragments on both sides of every threshold, for every
  svtype / strand arrangement.  tests/golden/make_golden.py:make_geometry_edges runs the REFERENCE over it and writes
  tests/golden/geometry_edges.json.gz.  No random draws except the MAPQs (fixed seed, never 0: a gated MAPQ must be visible).

Reads are emitted in the order a BAM fetch of region A, then region B delivers them (each by coordinate), so that the same
reads written to a coordinate-sorted BAM give the same fragments (which primary is readA depends on that order).
"""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional, Tuple

from fakereads import FakeRead, parse_cigar

M = 20            # min_aligned of every call
SLOP = 3          # split slop
RL = 101
FLANK_MAX = 450   # max(mean + 3 sd) over LIBS: the fetch flank, integral (the classic and the sso window agree)
SPACING = 20_000  # distance between the sites of one group: no read of one site lies in a window of another
REF_LENGTH = 4_000_000
OSPAN_REF_LENGTH = 2**32 - 1

# name, read groups, mean, sd, read length; mean + 3 sd = 450.0 (integral), 431.75 (fractional), 410.5 (ends in .5)
LIBS = [("lib0", ["rg0"], 300.0, 50.0, RL), ("lib1", ["rg1"], 310.25, 40.5, RL), ("lib2", ["rg2"], 320.5, 30.0, RL)]
CIS = ([0, 0], [-3, 5], [-50, 0], [0, 50])

# label, svtype, o1, o2, layout
ARRANGEMENTS = [
    ("DEL", "DEL", False, True, "same"), ("DUP", "DUP", True, False, "same"),
    ("INVff", "INV", False, False, "same"), ("INVrr", "INV", True, True, "same"),
    ("BNDfr", "BND", False, True, "same"), ("BNDrf", "BND", True, False, "same"),
    ("BNDff", "BND", False, False, "same"), ("BNDrr", "BND", True, True, "same"),
    ("XBNDfr", "BND", False, True, "inter"), ("XBNDrf", "BND", True, False, "inter_pos"),     # inter_pos: pos_a > pos_b
    ("XBNDff", "BND", False, False, "inter_tid"), ("XBNDrr", "BND", True, True, "inter"),    # inter_tid: tid_a > tid_b
]


def library_specs():
    """[(name, readgroups, mean, sd, read_length, hist)] in the shape fakereads.make_libraries returns (integer-only hist)"""
    return [(name, rgs, mean, sd, rl, {k: max(1, 400 - 2 * abs(k - int(mean))) for k in range(100, 601)})
            for (name, rgs, mean, sd, rl) in LIBS]


def flank_of(lib: int) -> float:
    return LIBS[lib][2] + LIBS[lib][3] * 3


def flank_class(flank: float) -> str:
    if flank == int(flank):
        return "int"
    return "half" if flank * 2 == int(flank * 2) else "frac"


# ============================================================================================ census
_ALIGNED = (0, 7, 8)        # M = X
_REF = (0, 2, 3, 7, 8)      # M D N = X
_CLIP = (4, 5)


def _end(start, cigar):
    return start + sum(n for op, n in cigar if op in _REF)


def intervals(read) -> List[Tuple[int, int]]:
    """maximal reference intervals covered by M/=/X bases with no D/N between them"""
    out, p, cur = [], read.reference_start, None
    for op, n in read.cigar:
        if op in _ALIGNED:
            cur = [p, p + n] if cur is None else [cur[0], p + n]
            p += n
        elif op in (2, 3):
            if cur is not None:
                out.append((cur[0], cur[1]))
                cur = None
            p += n
    if cur is not None:
        out.append((cur[0], cur[1]))
    return out


def overlap(read, start, end) -> int:
    """pysam's get_overlap: aligned (M/=/X) reference bases inside [start, end)"""
    ov, p = 0, read.reference_start
    for op, n in read.cigar:
        if op in _ALIGNED:
            ov += max(0, min(p + n, end) - max(p, start))
        if op in _REF:
            p += n
    return ov


def is_ref_seq(read, chrom, pos, m) -> bool:             # parsers.py:801-816
    if read.reference_name != chrom:
        return False
    if overlap(read, max(0, pos - m), pos + m) < 2 * m:
        return False
    return True


def _side(inner, pos, ci, rev, flank):
    """one side of parsers.py:846-855 -> (passes, [(kind, signed distance)])"""
    ev = []
    if not rev:
        ok = not (inner > pos + ci[1] or inner < pos + ci[0] - flank)
        near, far = inner - (pos + ci[1]), inner - math.ceil(pos + ci[0] - flank)
    else:
        ok = not (inner < pos + ci[0] or inner > pos + ci[1] + flank)
        near, far = inner - (pos + ci[0]), inner - math.floor(pos + ci[1] + flank)
    if abs(near) <= 2:
        ev.append(("near", near))
    if abs(far) <= 2:
        ev.append(("far", far))
    return ok, ev


def pair_straddle(prim, chromA, posA, ciA, chromB, posB, ciB, o1, o2, m, flank):
    """parsers.py:821-857 -> (verdict, events [(side, rev, kind, d, decisive)]); events only when orientation and
    chromosomes let the inner span be looked at"""
    if len(prim) != 2:
        return False, []
    a, b = prim
    if a.is_reverse != o1 or b.is_reverse != o2:
        return False, []
    if a.reference_name != chromA or b.reference_name != chromB:
        return False, []
    i1, i2 = a.reference_start + m, b.reference_end - m - 1       # get_ispan, :785-789
    ok1, ev1 = _side(i1, posA, ciA, o1, flank)
    ok2, ev2 = _side(i2, posB, ciB, o2, flank)
    events = [(1, o1, kind, d, ok2) for kind, d in ev1] + [(2, o2, kind, d, ok1) for kind, d in ev2]
    return ok1 and ok2, events


def _left_clip(cigar) -> bool:                                 # parsers.py:1242-1253
    l, r = cigar[0], cigar[-1]
    lc, rc = l[0] in _CLIP, r[0] in _CLIP
    return (lc and not rc) or (lc and rc and l[1] > r[1])


def split_candidate(read):
    """(kind, left piece, right piece) by shape, pieces as (chrom, start, end, mapq); ("two_sa", None, None) for a read with
    more than one SA entry; None for a read that is no candidate"""
    if not read.cigar:
        return None
    a = (read.reference_name, read.reference_start, read.reference_end, read.mapping_quality)
    if not read.has_tag("SA"):
        first, last = read.cigar[0], read.cigar[-1]
        clip = max(first[1] * (first[0] in _CLIP), last[1] * (last[0] in _CLIP))
        if clip > 0 and read.query_length - read.query_alignment_length <= 50:
            b = (None, 1, 1, 0)
            return ("clip", b, a) if _left_clip(read.cigar) else ("clip", a, b)
        return None
    entries = read.get_tag("SA").rstrip(";").split(";")
    if len(entries) > 1:
        return ("two_sa", None, None)
    f = entries[0].split(",")
    pos, cig = int(f[1]) - 1, parse_cigar(f[3])
    b = (f[0], pos, _end(pos, cig), int(f[4]))
    if read.reference_name == f[0]:
        return ("seq", b, a) if read.reference_start > pos else ("seq", a, b)
    return ("seq", b, a) if _left_clip(read.cigar) else ("seq", a, b)


def _support(piece, chrom, pos, rev, slop):                    # parsers.py:1122-1134
    if piece[0] != chrom:
        return False, None
    coord = piece[1] if rev else piece[2]
    return not (coord > pos + slop or coord < pos - slop), coord - pos


def split_straddle(kind, left, right, bp, slop):
    """parsers.py:1136-1215 -> (left verdict, right verdict, events [(piece, target, rev of target, d or None, verdict of the
    comparison, decisive)]); d is None for a piece on another chromosome than its target"""
    A, B = bp["A"], bp["B"]
    if A["chrom"] != B["chrom"] or A["pos"] > B["pos"]:
        lo, hi = ("B", B), ("A", A)
    else:
        lo, hi = ("A", A), ("B", B)
    soft, svtype = kind == "clip", bp["svtype"]
    if not soft or svtype in ("DEL", "INS"):
        plan = {"L": [lo], "R": [hi]}
    elif svtype == "DUP":
        plan = {"L": [hi], "R": [lo]}
    elif svtype == "INV":
        plan = {"L": [lo, hi], "R": [lo, hi]}
    else:
        plan = {"L": [], "R": []}
    verdict, events = {}, []
    for name, piece in (("L", left), ("R", right)):
        res = [(_support(piece, t["chrom"], t["pos"], t["is_reverse"], slop), side, t) for side, t in plan[name]]
        verdict[name] = any(ok for (ok, _), _, _ in res)
        for k, ((ok, d), side, t) in enumerate(res):
            others = any(o for j, ((o, _), _, _) in enumerate(res) if j != k)
            if piece[0] is not None:
                events.append((name, side, t["is_reverse"], d, ok, not others))
    return verdict["L"], verdict["R"], events


def arrangement_of(bp) -> tuple:
    A, B = bp["A"], bp["B"]
    if A["chrom"] == B["chrom"]:
        layout = "same" if A["pos"] <= B["pos"] else "same_pos"
    else:
        layout = "inter_tid" if A["chrom"] > B["chrom"] else ("inter_pos" if A["pos"] > B["pos"] else "inter")
    return (bp["svtype"], A["is_reverse"], B["is_reverse"], layout)


def group_fragments(reads):
    """{name: (primaries in order of arrival, all reads)} with the (name, flag) de-duplication of parsers.py:748-754"""
    frags: Dict[str, list] = {}
    seen = set()
    for r in reads:
        if (r.query_name, r.flag) in seen:
            continue
        seen.add((r.query_name, r.flag))
        frags.setdefault(r.query_name, [])
        if not r.is_supplementary and not r.is_secondary:
            frags[r.query_name].append(r)
    return frags


def census(bp, reads, lib_of_rg: Dict[str, float], m=M, slop=SLOP):
    """Per fragment in sorted(name) order: {"name", "rs": [verdict per primary], "alt", "ref_a", "ref_b" (None without a
    pair), "splits": [(kind, left verdict, right verdict)], "events": [(key, field, verdict, decisive)]}.

    `lib_of_rg`: read group -> mean + 3 sd of its library.  An event's `field` names where the reference's record shows the
    verdict (("flag", bit) of the first record, ("rs", primary index), (kind, "L" / "R", candidate index)); `decisive` says
    that no other comparison sets the same field, so the field equals the verdict."""
    A, B = bp["A"], bp["B"]
    o1, o2 = A["is_reverse"], B["is_reverse"]
    out = []
    frags = group_fragments(reads)
    for name in sorted(frags):
        prim = frags[name]
        flank = lib_of_rg[prim[0].get_tag("RG")] if prim else 0.0
        fc = flank_class(flank)
        events = []
        # ---- is_ref_seq per primary, both breakends
        rs = []
        for j, r in enumerate(prim):
            hits = {s: is_ref_seq(r, bp[s]["chrom"], bp[s]["pos"], m) for s in ("A", "B")}
            rs.append(hits["A"] or hits["B"])
            for s in ("A", "B"):
                if r.reference_name != bp[s]["chrom"]:
                    continue
                pos = bp[s]["pos"]
                dec = not hits["B" if s == "A" else "A"]
                lo, hi = pos - m, pos + m
                if lo <= 1 and r.reference_start <= 2:
                    events.append((("ref_seq_start_of_chrom", lo, r.reference_start), ("rs", j), hits[s], dec))
                    continue
                ivs = intervals(r)
                eqx = any(op in (7, 8) for op, _ in r.cigar)
                for k, (s0, e0) in enumerate(ivs):
                    tag = (k + 1, len(ivs), "eqx" if eqx else "m")
                    if abs(s0 - lo) <= 2 and e0 >= hi + 3:
                        events.append((("ref_seq", s, min(j, 2), "start", s0 - lo) + tag, ("rs", j), hits[s], dec))
                    if abs(e0 - hi) <= 2 and s0 <= lo - 3:
                        events.append((("ref_seq", s, min(j, 2), "end", e0 - hi) + tag, ("rs", j), hits[s], dec))
                    if s0 <= lo - 3 and e0 >= hi + 3:
                        p, ins = r.reference_start, False
                        for op, n in r.cigar:
                            if op == 1 and lo < p < hi:
                                ins = True
                            if op in _REF:
                                p += n
                        events.append((("ref_seq", s, min(j, 2), "inside_ins" if ins else "inside", 0) + tag, ("rs", j), hits[s], dec))
        # ---- the pair
        alt = ref_a = ref_b = None
        if len(prim) == 2:
            alt1, ev1 = pair_straddle(prim, A["chrom"], A["pos"], A["ci"], B["chrom"], B["pos"], B["ci"], o1, o2, m, flank)
            alt2, ev2 = False, []
            if bp["svtype"] == "INV":                                  # classic.py:349-357 (asked when the first is False)
                alt2, ev2 = pair_straddle(prim, A["chrom"], A["pos"], A["ci"], B["chrom"], B["pos"], B["ci"], not o1, not o2, m, flank)
            alt = alt1 or alt2
            for pred, evs, other in (("alt", ev1, alt2), ("alt_recip", ev2, alt1)):
                for side, rev, kind, d, dec in evs:
                    ci = tuple(A["ci"] if side == 1 else B["ci"])
                    events.append(((pred, side, rev, kind, d, ci, fc if kind == "far" else None), ("flag", 1), None, dec and not other))
            ref_a, ev = pair_straddle(prim, A["chrom"], A["pos"], [0, 0], A["chrom"], A["pos"], [0, 0], False, True, m, flank)
            events += [(("ref_a", side, rev, kind, d, (0, 0), fc if kind == "far" else None), ("flag", 2), None, dec) for side, rev, kind, d, dec in ev]
            ref_b, ev = pair_straddle(prim, B["chrom"], B["pos"], [0, 0], B["chrom"], B["pos"], [0, 0], False, True, m, flank)
            events += [(("ref_b", side, rev, kind, d, (0, 0), fc if kind == "far" else None), ("flag", 4), None, dec) for side, rev, kind, d, dec in ev]
            fixed = {1: alt, 2: ref_a, 4: ref_b}
            events = [(k, f, fixed[f[1]] if f[0] == "flag" else v, dec) for k, f, v, dec in events]
        # ---- split candidates, in the order of the primaries
        splits, n_kind = [], {"seq": 0, "clip": 0}
        for r in prim:
            cand = split_candidate(r)
            if cand is None:
                continue
            kind, left, right = cand
            if kind == "two_sa":
                events.append((("split_two_sa",), ("none", None, None), False, True))
                continue
            lv, rv, evs = split_straddle(kind, left, right, bp, slop)
            idx = n_kind[kind]
            n_kind[kind] += 1
            splits.append((kind, lv, rv))
            for piece, side, rev, d, ok, dec in evs:
                if d is None:
                    events.append((("split_wrong_chrom", kind, piece), (kind, piece, idx), lv if piece == "L" else rv, dec))
                elif abs(d) <= 6:
                    events.append((("split", kind, piece, side, rev, d), (kind, piece, idx), ok, dec))
        out.append({"name": name, "n_primary": len(prim), "rs": rs, "alt": alt, "ref_a": ref_a, "ref_b": ref_b,
                    "splits": splits, "events": events})
    return out


ROW = {"ospan": 0, "mq_a": 1, "mq_b": 2, "rs_a": 3, "rs_b": 4, "seq_l": 5, "seq_r": 6, "clip_l": 7, "clip_r": 8, "flags": 9}


def field_value(rows, field) -> bool:
    """does the reference's record show `field` (see census) as set; `rows`: the fragment's record rows, first one first"""
    what = field[0]
    if what == "flag":
        return bool(rows[0][ROW["flags"]] & field[1])
    if what == "rs":
        j = field[1]
        return rows[j // 2][ROW["rs_a"] + (j % 2)] > 0
    if what == "none":
        return any(x for row in rows for x in row[ROW["seq_l"]:ROW["clip_r"] + 1])
    kind, piece, idx = field
    return rows[idx][ROW["%s_%s" % (kind, piece.lower())]] > 0


def site_census(site, libraries_json, fh=float.fromhex):
    """census of one site of a golden file (fake_sites.json.gz / geometry_edges.json.gz)"""
    lib_of_rg = {rg: fh(L["mean"]) + fh(L["sd"]) * 3 for L in libraries_json for rg in L["readgroups"]}
    return census(site["breakpoint"], [FakeRead(*t) for t in site["reads"]], lib_of_rg)


def event_table(golden) -> Dict[tuple, int]:
    """event key (without the site's arrangement) -> number of decisive events, over a whole golden file"""
    table: Dict[tuple, int] = {}
    for grp in golden["groups"]:
        for site in grp["sites"]:
            for frag in site_census(site, grp["libraries"]):
                for key, _field, verdict, dec in frag["events"]:
                    if dec:
                        table[key + (verdict,)] = table.get(key + (verdict,), 0) + 1
    return table


# ============================================================================================ corpus
class _Site:
    def __init__(self, sid, bp, rng, shared=False):
        self.id, self.bp, self.rng, self.shared = sid, bp, rng, shared
        self.reads: List[FakeRead] = []
        self.n = 0

    def mq(self):
        return self.rng.choice([60, 60, 60, 37, 20, 1, 255, 59])

    def name(self, tag):
        self.n += 1
        return "%s.%s%03d" % (self.id, tag, self.n)

    def read(self, name, flag, chrom, start, cigar, lib=0, sa=None):
        qlen = sum(n for op, n in parse_cigar(cigar) if op in (0, 1, 4, 7, 8))
        r = FakeRead(name, flag, chrom, start, cigar, self.mq(), sa=sa, rg="rg%d" % lib, query_length=qlen)
        self.reads.append(r)
        return r

    def pair(self, tag, chrom_a, a_start, a_rev, chrom_b, b_end, b_rev, lib=0, a_cigar="101M", b_cigar="101M"):
        """first read starts at a_start, second read ENDS at b_end"""
        name = self.name(tag)
        b_start = b_end - sum(n for op, n in parse_cigar(b_cigar) if op in _REF)
        self.read(name, 65 | (0x10 if a_rev else 0) | (0x20 if b_rev else 0), chrom_a, a_start, a_cigar, lib)
        self.read(name, 129 | (0x10 if b_rev else 0) | (0x20 if a_rev else 0), chrom_b, b_start, b_cigar, lib)
        return name

    def windows(self):
        return [(self.bp[s]["chrom"], max(self.bp[s]["pos"] + self.bp[s]["ci"][0] - FLANK_MAX, 0),
                 self.bp[s]["pos"] + self.bp[s]["ci"][1] + FLANK_MAX) for s in ("A", "B")]

    def fetch_order(self, check=True):
        """the reads as a fetch of window A, then of window B delivers them from a coordinate-sorted file"""
        order, taken = [], set()
        for chrom, lo, hi in self.windows():
            hit = [k for k, r in enumerate(self.reads) if r.reference_name == chrom and r.reference_start < hi - 2
                   and r.reference_end > lo + 2 and k not in taken]
            hit.sort(key=lambda k: self.reads[k].reference_start)
            order += hit
            taken.update(hit)
        if check and len(order) != len(self.reads):
            missing = [self.reads[k].astuple() for k in range(len(self.reads)) if k not in taken]
            raise AssertionError("site %s: reads outside both fetch windows: %r" % (self.id, missing[:3]))
        return [self.reads[k] for k in order]


def _breakpoint(sid, svtype, o1, o2, layout, ci_a, ci_b, base, gap=3000):
    if layout == "same":
        a, b = ("1", base), ("1", base + gap)
    elif layout == "inter":
        a, b = ("1", base), ("2", base + gap)
    elif layout == "inter_pos":
        a, b = ("1", base + 2 * gap), ("2", base)
    else:
        a, b = ("2", base), ("1", base + gap)
    bp = {"id": sid, "svtype": svtype,
          "A": {"chrom": a[0], "pos": a[1], "ci": list(ci_a), "is_reverse": o1},
          "B": {"chrom": b[0], "pos": b[1], "ci": list(ci_b), "is_reverse": o2}}
    if svtype == "DEL":
        bp["var_length"] = b[1] - a[1]
    return bp


def _far_inner(pos, ci, rev, lib, d):
    return (math.floor(pos + ci[1] + flank_of(lib)) if rev else math.ceil(pos + ci[0] - flank_of(lib))) + d


def _inside(pos, ci, rev):
    return pos + ci[1] + 100 if rev else pos + ci[0] - 100


def _pair_lattice(site, tag, A, B, ciA, ciB, o1, o2):
    """pairs whose inner span sits on the thresholds of one side, the other side comfortably inside"""
    for side in (1, 2):
        pos, ci, rev = (A["pos"], ciA, o1) if side == 1 else (B["pos"], ciB, o2)
        inners = [(pos + ci[0] - 1, 0), (pos + ci[0], 0), (pos + ci[1], 0), (pos + ci[1] + 1, 0)]
        inners += [(_far_inner(pos, ci, rev, lib, d), lib) for lib in range(len(LIBS)) for d in (-1, 0, 1)]
        for inner, lib in inners:
            i1 = inner if side == 1 else _inside(A["pos"], ciA, o1)
            i2 = inner if side == 2 else _inside(B["pos"], ciB, o2)
            site.pair(tag, A["chrom"], i1 - M, o1, B["chrom"], i2 + M + 1, o2, lib)


def _sites_of(label, svtype, o1, o2, layout, slot, rng):
    sites = []
    # ---- pair_straddle: one site per CI (side A has CIS[k], side B the next one)
    for k, ci in enumerate(CIS):
        ci_b = CIS[(k + 1) % len(CIS)]
        s = _Site("%s.ps%d" % (label, k), _breakpoint("%s.ps%d" % (label, k), svtype, o1, o2, layout, ci, ci_b, slot()), rng)
        A, B = s.bp["A"], s.bp["B"]
        _pair_lattice(s, "p", A, B, A["ci"], B["ci"], o1, o2)
        if svtype == "INV":
            _pair_lattice(s, "q", A, B, A["ci"], B["ci"], not o1, not o2)
        sites.append(s)
    # ---- reference straddles at A and at B: CI ignored, orientation (+, -)
    s = _Site(label + ".ref", _breakpoint(label + ".ref", svtype, o1, o2, layout, [-3, 5], [-3, 5], slot()), rng)
    for side in ("A", "B"):
        X = s.bp[side]
        _pair_lattice(s, "r" + side.lower(), X, X, [0, 0], [0, 0], False, True)
    sites.append(s)
    # ---- is_ref_seq: both reads of the pair, both breakends, the window's two ends
    s = _Site(label + ".rs", _breakpoint(label + ".rs", svtype, o1, o2, layout, [0, 0], [0, 0], slot()), rng)
    for side in ("A", "B"):
        X = s.bp[side]
        c, pos = X["chrom"], X["pos"]
        for d in (-1, 0, 1):
            for start in (pos - M + d, pos + M + d - RL):          # interval starts at pos - m + d / ends at pos + m + d
                s.pair("a", c, start, False, c, pos + 150 + RL, True)           # the read under test comes first
                s.pair("b", c, pos - 300, False, c, start + RL, True)           # ... and second
    sites.append(s)
    # ---- split and clip: coord - pos in -5 .. +5
    s = _Site(label + ".sp", _breakpoint(label + ".sp", svtype, o1, o2, layout, [0, 0], [0, 0], slot()), rng)
    strand = "+" if o1 != o2 else "-"
    for side in ("A", "B"):
        X, Q = s.bp[side], s.bp["B" if side == "A" else "A"]
        for d in range(-5, 6):
            for cigar in ("60M41S", "41S60M"):          # soft clip without SA; the coordinate the side looks at is pos + d
                start = X["pos"] + d if X["is_reverse"] else X["pos"] + d - 60
                s.read(s.name("c"), 65, X["chrom"], start, cigar)
            for vary in ("P", "Q"):                     # primary piece at X, SA piece at the other breakend
                dp, dq = (d, 0) if vary == "P" else (0, d)
                pcig = "51S50M" if X["is_reverse"] else "50M51S"
                pstart = X["pos"] + dp if X["is_reverse"] else X["pos"] + dp - 50
                qcig = "50S51M" if Q["is_reverse"] else "51M50S"
                qstart = Q["pos"] + dq if Q["is_reverse"] else Q["pos"] + dq - 51
                sa = "%s,%d,%s,%s,%d,0;" % (Q["chrom"], qstart + 1, strand, qcig, s.mq())
                s.read(s.name("s"), 65, X["chrom"], pstart, pcig, sa=sa)
    A, B = s.bp["A"], s.bp["B"]
    pcig, pstart = ("51S50M", A["pos"]) if o1 else ("50M51S", A["pos"] - 50)
    qcig, qstart = ("50S51M", B["pos"]) if o2 else ("51M50S", B["pos"] - 51)
    other = "2" if B["chrom"] == "1" else "1"
    s.read(s.name("w"), 65, A["chrom"], pstart, pcig, sa="%s,%d,%s,%s,60,0;" % (other, qstart + 1, strand, qcig))   # wrong chromosome
    s.read(s.name("t"), 65, A["chrom"], pstart, pcig,                                                                # two SA entries
           sa="%s,%d,%s,%s,60,0;%s,%d,+,50M51S,30,0;" % (B["chrom"], qstart + 1, strand, qcig, A["chrom"], A["pos"] + 200))
    sites.append(s)
    return sites


def _special_sites(slot, rng):
    sites = []
    # ---- a pair that straddles A and B at once (breakends 200 apart)
    s = _Site("both", _breakpoint("both", "DEL", False, True, "same", [0, 0], [0, 0], slot(), gap=200), rng)
    A, B = s.bp["A"], s.bp["B"]
    for lib in range(len(LIBS)):
        s.pair("p", "1", A["pos"] - 50 - M, False, "1", B["pos"] + 50 + M + 1, True, lib)
        s.pair("p", "1", A["pos"] - 50 - M, False, "1", A["pos"] + 50 + M + 1, True, lib)      # A only
    sites.append(s)
    # ---- CIGARs: second interval behind N and D, an insertion inside the window, = / X, four intervals
    s = _Site("cigar", _breakpoint("cigar", "DEL", False, True, "same", [0, 0], [0, 0], slot()), rng)
    P = s.bp["A"]["pos"]
    mate = P + 300 + RL
    for d in (-1, 0, 1):
        s.pair("n", "1", P - M + d - 150, False, "1", mate, True, a_cigar="50M100N51M")      # second interval starts at pos - m + d
        s.pair("d", "1", P - M + d - 55, False, "1", mate, True, a_cigar="50M5D51M")
        s.pair("n", "1", P + M + d - 50, False, "1", mate, True, a_cigar="50M100N51M")       # first interval ends at pos + m + d
        s.pair("d", "1", P + M + d - 50, False, "1", mate, True, a_cigar="50M5D51M")
        s.pair("x", "1", P - M + d, False, "1", mate, True, a_cigar="40=1X60=")
        s.pair("x", "1", P + M + d - RL, False, "1", mate, True, a_cigar="40=1X60=")
        s.pair("f", "1", P - M + d - 80, False, "1", mate, True, a_cigar="30M10N30M10N50M10N30M")   # third of four starts there
        s.pair("f", "1", P + M + d - 130, False, "1", mate, True, a_cigar="30M10N30M10N50M10N30M")  # ... ends there
    s.pair("i", "1", P - 30, False, "1", mate, True, a_cigar="30M2I69M")                     # insertion at pos, interval contiguous
    s.pair("f", "1", P - 105, False, "1", mate, True, a_cigar="30M10N30M10N50M10N30M")       # window in the middle of the third
    sites.append(s)
    # ---- four intervals, the two nearest to the breakends (100 apart) are the 2nd and the 4th
    s = _Site("iv4", _breakpoint("iv4", "DEL", False, True, "same", [0, 0], [0, 0], slot(), gap=100), rng)
    P = s.bp["A"]["pos"]
    s.pair("b", "1", P - 45, False, "1", P + 400, True, a_cigar="30M10N50M10N10M10N50M")     # B's window inside the 4th, A's not inside the 2nd
    s.pair("a", "1", P - 65, False, "1", P + 400, True, a_cigar="30M10N50M10N10M10N50M")     # A's window inside the 2nd, B's not inside the 4th
    s.pair("z", "1", P - 95, False, "1", P + 400, True, a_cigar="30M10N50M10N10M10N50M")     # neither
    sites.append(s)
    # ---- counts: three primaries, the same record twice, two soft clips in one fragment (a continuation record)
    s = _Site("counts", _breakpoint("counts", "DEL", False, True, "same", [0, 0], [0, 0], slot()), rng)
    A, B = s.bp["A"], s.bp["B"]
    name = s.pair("t", "1", A["pos"] - 200, False, "1", A["pos"] + 60, True)
    s.read(name, 73, "1", A["pos"] - M, "101M")                                              # third primary (the last to arrive), on A's window
    name = s.pair("w", "1", A["pos"] - 150, False, "1", A["pos"] + 200, True)
    first = s.reads[-2]
    s.reads.append(FakeRead(*first.astuple()))                                               # the same record again
    name = s.name("k")
    s.read(name, 65 | 0x20, "1", A["pos"] - 60, "60M41S")
    s.read(name, 129 | 0x10, "1", B["pos"], "41S60M")
    s.read(s.name("o"), 73, "1", A["pos"] - M, "101M")                                       # one primary
    sites.append(s)
    return sites


def _chrom_start_sites(rng):
    """pos = m - 1, m, m + 1 at the start of chromosome 2: the reference's max(0, pos - m) shortens the window.  The three
    sites share their reads (their windows are the same stretch of the chromosome)."""
    sites = []
    for k, pos in enumerate((M - 1, M, M + 1)):
        bp = {"id": "start%d" % pos, "svtype": "DEL", "var_length": 3000,
              "A": {"chrom": "2", "pos": pos, "ci": [0, 0], "is_reverse": False},
              "B": {"chrom": "2", "pos": pos + 3000, "ci": [0, 0], "is_reverse": True}}
        s = _Site("start", bp, random.Random(7), shared=k > 0)      # (the same MAPQs for the three)
        for start in (0, 1, 2):
            s.pair("a", "2", start, False, "2", 300 + RL, True)
        s.pair("g", "2", 0, False, "2", 300 + RL, True, a_cigar="41M10N50M")
        s.id = bp["id"]
        sites.append(s)
    return sites


def _empty(sid, slot):
    return _Site(sid, _breakpoint(sid, "DEL", False, True, "same", [0, 0], [0, 0], slot()), None)


def corpus():
    """[{"name", "bam" (can the group be written as a BAM), "ref_length", "sites": [{"breakpoint", "reads" (FakeRead, fetch
    order), "shared_reads", "fits_int32"}]}]"""
    rng = random.Random(20261018)
    counter = [0]

    def slot():
        counter[0] += 1
        return 100_000 + SPACING * counter[0]

    sites = [_empty("empty.lead", slot)]
    for k, (label, svtype, o1, o2, layout) in enumerate(ARRANGEMENTS):
        sites += _sites_of(label, svtype, o1, o2, layout, slot, rng)
        if k == 5:
            sites += [_empty("empty.mid1", slot), _empty("empty.mid2", slot)]
    sites += _special_sites(slot, rng)
    sites += _chrom_start_sites(rng)
    sites.append(_empty("empty.trail", slot))
    assert 100_000 + SPACING * (counter[0] + 1) < REF_LENGTH
    main = {"name": "lattice", "bam": True, "ref_length": REF_LENGTH,
            "sites": [{"breakpoint": s.bp, "reads": s.fetch_order(), "shared_reads": s.shared, "fits_int32": True} for s in sites]}

    # ---- ospan: |b.end - a.start| = 2^31 - 2, 2^31 - 1, 2^31 + 5 on a chromosome of 2^32 - 1 bases (no BAM can carry these)
    osites = []
    for k, span in enumerate((2**31 - 2, 2**31 - 1, 2**31 + 5)):
        s = _Site("ospan%d" % k, _breakpoint("ospan%d" % k, "DEL", False, True, "same", [0, 0], [0, 0], 1000), rng)
        s.pair("o", "1", 0, False, "1", span, True)
        osites.append({"breakpoint": s.bp, "reads": list(s.reads), "shared_reads": False, "fits_int32": span <= 2**31 - 1})
    ospan = {"name": "ospan", "bam": False, "ref_length": OSPAN_REF_LENGTH, "sites": osites}
    return [main, ospan]


# pos_a of the units of the kernel's unit look-up test -> what its one pair (first read [1000, 1101) forward, second read
# [1300, 1401) reverse) shows against it: rs_a + ref A, ref A, rs_b + ref A, rs_b, nothing
LOOKUP_POS_A = [1050, 1200, 1350, 1381, 1010]


# ============================================================================================ golden -> inputs of the tests
def bam_records(group):
    """bamwriter records of one golden group, sorted by position (stable: reads at one position keep their fetch order)"""
    tid_of = {"1": 0, "2": 1}
    recs = []
    for site in group["sites"]:
        if site["shared_reads"]:
            continue
        for (name, flag, ref, start, cigar, mapq, sa, rg, _qlen, tlen) in site["reads"]:
            tags = [("RG", "Z", rg)] + ([("SA", "Z", sa)] if sa else [])
            recs.append(dict(name=name, flag=flag, tid=tid_of[ref], pos=start, mapq=mapq, cigar=cigar, mtid=tid_of[ref],
                             mpos=start, tlen=tlen, tags=tags))
    recs.sort(key=lambda r: (r["tid"], r["pos"]))
    return recs


def write_group_bam(tmp_path, group, libraries_json, block_bytes=2500):
    """(sites, sample, nbam) of one group of geometry_edges.json.gz written with tests/bamwriter.py"""
    import bamwriter as bw
    import walkcases as W
    n = group["ref_length"]
    header = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:1\tLN:%d\n@SQ\tSN:2\tLN:%d\n" % (n, n) + "".join(
        "@RG\tID:%s\tSM:edges\tLB:%s\n" % (rg, L["name"]) for L in libraries_json for rg in L["readgroups"])
    recs = bam_records(group)
    path = str(tmp_path / ("edges_%s.bam" % group["name"]))
    bw.write_bam(path, header, [("1", n), ("2", n)], recs, block_bytes=block_bytes)
    fh = float.fromhex
    info = {"edges": {"mapped": len(recs), "unmapped": 0, "bam": path, "sample_name": "edges", "libraryArray": [
        {"library_name": L["name"], "readgroups": L["readgroups"], "read_length": L["read_length"], "histogram": L["hist"],
         "mean": fh(L["mean"]), "sd": fh(L["sd"]), "prevalence": 1.0 / len(libraries_json)} for L in libraries_json]}}
    sample, nbam = W.open_sample(path, info)
    return [{"breakpoint": s["breakpoint"]} for s in group["sites"]], sample, nbam

#!/usr/bin/env python
"""Generate tests/golden/concordance_edges.json.gz by IMPORTING THE REFERENCE (dev container only).

    python tests/golden/make_golden_concordance.py

The lattice of tests/concordcases.py through the reference's own SamFragment.p_concordant (parsers.py:861-882): per library a
reference Library is built from the histogram (its `dens` left for the reference to compute, parsers.py:579-583) and asked, at
every point (ospan_len, var_length or None), through a SamFragment subclass whose get_ospan returns (0, ospan_len).

    "libraries"  the small families, in concordcases.small_libraries() order: family, name, hist, mean and sd (hex floats),
                 points [[ospan_len, var_length or null]] and answers, a string of '0' / '1', one per point
    "wide"       the formula-made libraries: the recipe's name, the SHA-256 of the histogram (little-endian uint32 counts),
                 key_min, the number of bins and points, and the answers; histogram and points come from concordcases
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refload  # noqa: E402
import make_golden as MG  # noqa: E402
import concordcases as CC  # noqa: E402

NAME = "concordance_edges.json.gz"


def answers(ref, hist, mean, sd, points):
    lib = ref.parsers.Library("lib", None, ["rg"], 101, dict(hist), None, mean, sd, 1.0, 0)

    class Span(ref.parsers.SamFragment):
        def __init__(self, ospan_len):             # (no reads: p_concordant reads the library and the outer span only)
            self.lib = lib
            self.ospan_len = ospan_len

        def get_ospan(self):
            return (0, self.ospan_len)

    out = []
    for o, v in points:
        got = Span(o).p_concordant(v)
        assert got is True or got is False
        out.append("1" if got else "0")
    return "".join(out)


def make_concordance(ref):
    libraries = []
    for L in CC.small_libraries():
        libraries.append({"family": L.family, "name": L.name, "hist": {str(k): int(c) for k, c in L.hist.items()}, "mean": MG.hx(L.mean),
                          "sd": MG.hx(L.sd), "points": [[o, v] for o, v in L.points], "answers": answers(ref, L.hist, L.mean, L.sd, L.points)})
    wide = []
    for recipe in CC.WIDE_RECIPES:
        L = CC.wide_library(recipe)
        hist = {CC.WIDE_KEY_MIN + i: int(c) for i, c in enumerate(L.counts.tolist())}
        wide.append({"recipe": recipe, "sha256": CC.wide_sha256(recipe), "key_min": CC.WIDE_KEY_MIN, "n_bins": len(hist), "mean": MG.hx(L.mean),
                     "sd": MG.hx(L.sd), "n_points": len(L.points), "answers": answers(ref, hist, L.mean, L.sd, L.points)})
    MG.dump(NAME, {"libraries": libraries, "wide": wide})


if __name__ == "__main__":
    make_concordance(refload.load_reference())

#!/usr/bin/env python
"""Writes the units tools/reader_time.cpp reads: the fixture's sites x REPEAT as windows.bin + breakpoints.bin in DIR, and
prints the rest of reader_time's command line.  usage: dump_units.py DIR [REPEAT=100]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import walkcases as W  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402

out, repeat = sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 100
sites, sample, nbam = W.fixture_input()
win, bps, rgs, rg_lib, _ = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
np.tile(win, repeat).tofile(os.path.join(out, "windows.bin"))
np.tile(bps, repeat).tofile(os.path.join(out, "breakpoints.bin"))
print(W.FIXTURE_BAM, os.path.join(out, "windows.bin"), os.path.join(out, "breakpoints.bin"), "THREADS REPS",
      " ".join("%s=%d" % (rg, lib) for rg, lib in zip(rgs, rg_lib)))

#!/usr/bin/env python
"""Generate tests/golden/long_contig_sites.json.gz by IMPORTING THE REFERENCE (dev container only), as make_golden.py's
make_fake does for fake_sites.json.gz.

    python tests/golden/make_golden_long_contig.py

Three groups of 20 tests/fakereads.py::make_site sites on two contigs of length 2^31 - 1.  In group k every read start, every
SA position and both breakpoint positions of a site are shifted by K[k]:

    2^29 - 110 000     sites on both sides of 2^29: where a BAI ends, and the boundary between the first two top-level bins
                       of a depth-6 CSI
    3 * 2^29 + 12 345  well inside the range only a CSI addresses
    2^31 - 2^20        every position stays more than 700 000 below 2^31, so no window arithmetic of the reference leaves int32

A read's query_length is the l_seq of its BAM record (see shifted()).  Per site: `breakpoint`, `reads`, `records`,
`tallies_sso` and `result`, exactly as make_fake records them (the reference's fragment objects and predicates over the reads
themselves).  The tests write each group as ONE BAM and read the sites back through the index, so a site is kept only if a
reader of that BAM is handed the reads the reference was handed here: every read of the site overlaps one of the site's two
fetch windows (singlesample.py:139-156), and no read of another site of the group does.  Both conditions are decided from the
drawn coordinates alone; make_site is called until 20 sites are kept (`drawn` in the file says how many it took).
"""
from __future__ import annotations

import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refload  # noqa: E402
import fakereads  # noqa: E402
import make_golden as MG  # noqa: E402
from svtyper_amd import bam as bam_module  # noqa: E402
from svtyper_amd import packer  # noqa: E402

NAME = "long_contig_sites.json.gz"
SEED = 20261018
REF_LENGTH = 2 ** 31 - 1
SHIFTS = (2 ** 29 - 110_000, 3 * 2 ** 29 + 12_345, 2 ** 31 - 2 ** 20)
SITES_PER_GROUP = 20
Z = 3


def shifted(bp, reads, k):
    """the site with every read start, SA position and breakpoint position moved up by k -- and every read's query_length set to
    the l_seq a BAM record of its CIGAR carries (make_site leaves it 0 or draws it freely, which no BAM written from the
    reads can say: the soft-clip rule, parsers.py:1031-1040, reads it)"""
    bp = dict(bp, A=dict(bp["A"], pos=bp["A"]["pos"] + k), B=dict(bp["B"], pos=bp["B"]["pos"] + k))
    out = []
    for r in reads:
        name, flag, ref, start, cigar, mapq, sa, rg, qlen, tlen = r.astuple()
        if sa:
            entries = [e.split(",") for e in sa.split(";") if e]
            sa = "".join(",".join([e[0], str(int(e[1]) + k)] + e[2:]) + ";" for e in entries)
        out.append(fakereads.FakeRead(name, flag, ref, start + k, cigar, mapq, sa, rg, r.infer_query_length(), tlen))
    return bp, out


def windows(bp, flank):
    """the two fetch regions of the reference (singlesample.py:139-156): (chrom, lo, hi)"""
    out = []
    for side in ("A", "B"):
        pos, ci = bp[side]["pos"], bp[side]["ci"]
        out.append((bp[side]["chrom"], int(max(pos + ci[0] - flank, 0)), int(min(pos + ci[1] + flank, REF_LENGTH))))
    return out


def fetched(read, wins):
    """pysam's overlap rule: pos < hi and reference end > lo"""
    end = max(read.reference_end, read.reference_start + 1)
    return any(read.reference_name == c and read.reference_start < hi and end > lo for c, lo, hi in wins)


def make_long_contig(ref):
    rng = random.Random(SEED)
    groups = []
    for g, k in enumerate(SHIFTS):
        libs = fakereads.make_libraries(rng, (1, 2, 3)[g])
        flank = max(mean + Z * sd for (_n, _r, mean, sd, _l, _h) in libs)            # Sample.get_fetch_flank(3)
        ref_libs = [ref.parsers.Library(name, None, rgs, rl, dict(hist), None, mean, sd, 1.0, 0)
                    for (name, rgs, mean, sd, rl, hist) in libs]
        rg_to_lib = {rg: L for L, spec in zip(ref_libs, libs) for rg in spec[1]}
        libs_json, lib_index = MG.lib_tables(ref_libs)
        kept, sites, drawn = [], [], 0
        while len(sites) < SITES_PER_GROUP:
            bp, reads = shifted(*fakereads.make_site(rng, "L%d_%d" % (g, drawn), libs), k)
            drawn += 1
            wins = windows(bp, flank)
            if not all(fetched(r, wins) for r in reads):
                continue
            if any(fetched(r, theirs) for _b, _r, theirs in kept for r in reads) or any(fetched(r, wins) for _b, others, _w in kept for r in others):
                continue
            kept.append((bp, reads, wins))
            frags = {}
            for r in reads:                      # as gather_reads does (singlesample.py:194-203)
                lib = rg_to_lib[r.get_tag("RG")]
                if r.query_name in frags:
                    frags[r.query_name].add_read(r)
                else:
                    frags[r.query_name] = ref.parsers.SamFragment(r, lib)
            recs = packer.pack_fragments(frags, bp, lib_index, 20, 3)
            counts = ref.singlesample.tally_variant_read_fragments(3, 20, bp, frags, False)
            if sum(counts.values()) == 0:
                result = MG.blank_like(ref)
            else:
                result = MG.result_to_json(ref.singlesample.bayesian_genotype(bp, counts, 1, 1, False))
            sites.append({
                "breakpoint": bp,
                "reads": [list(r.astuple()) for r in reads],
                "records": [[int(x) for x in row] for row in recs.tolist()],
                "tallies_sso": {t: MG.hx(counts[t]) for t in MG.TALLIES},
                "result": result,
            })
        groups.append({"shift": k, "drawn": drawn, "libraries": libs_json, "sites": sites})
    MG.dump(NAME, {"groups": groups, "read_fields": list(fakereads.READ_FIELDS), "ref_length": REF_LENGTH,
                   "min_aligned": 20, "split_slop": 3})


if __name__ == "__main__":
    make_long_contig(refload.load_reference(pysam_module=bam_module))

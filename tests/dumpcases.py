"""The edge corpus of the evidence dump (`svtyper -w` with the device reader) -- TEST INFRASTRUCTURE shared by
tests/test_write_alignment_dump_corpus.py (CPU: svt_bam_evidence_dump_walk_host), tests/test_write_alignment_device_reader.py
(GPU: svt_bam_evidence_device_dump) and tests/test_dump_rules_native.py (the rules under AddressSanitizer).

One library, four DEL sites on chromosome 1 (walkcases.HEADER / INFO): an empty first unit, the main unit around 50 050 / 50 851,
a small unit around 70 050 / 70 851, an empty last unit.  What the corpus has to reach is asserted by the CPU test from the
Python route's output alone (reach()).  Every read of a unit carries RG (neither reader takes one without) and a tag field takes at
least four bytes, so the tag areas of the corpus are 6 bytes and 10 bytes up; the shorter areas -- and every truncated prefix --
are the native test's, which hands records to the rules directly."""
import json

import bamwriter as bw
import deepcases as DC
import walkcases as WC

RG = ("RG", "Z", "rg")
A0, B0 = 50_050, 50_851          # the main unit's breakends (walkcases.SITE)
SEQ_SA = "1,50852,+,60S40M,60,0;"
N_DEEP = DC.BOUNDARIES[1]         # 1 025 reads of distinct names on top of the corpus: the main unit is beyond the on-chip tier

# the XV decorations of a read's tag area, by name: (tags in front of RG, tags behind RG)
XV_KINDS = {
    "none": ([], []),
    "z_last": ([], [("XV", "Z", "R")]),
    "z_first": ([("XV", "Z", "A")], []),
    "a_type": ([], [("XV", "A", "R"), ("NM", "C", 3)]),
    "twice": ([("XV", "Z", "R")], [("NM", "C", 1), ("XV", "A", "A")]),
    "array_behind": ([], [("XV", "Z", "R"), ("XB", "B", ("s", [1, -2, 3]))]),
    "only_besides_rg": ([], [("XV", "i", 7)]),
}
KINDS = list(XV_KINDS)


def _read(name, pos, flag=0x41, cigar="100M", mapq=60, xv="none", pad=None, extra=()):
    front, behind = XV_KINDS[xv]
    tags = list(front) + [RG] + list(behind) + list(extra)
    if pad is not None:
        tags.append(("XP", "Z", "p" * pad))
    return dict(name=name, flag=flag, tid=0, pos=pos, mapq=mapq, cigar=cigar, mtid=0, mpos=pos + 300, tlen=400, tags=tags, xv_kind=xv)


AREAS = [6] + list(range(10, 73))


def tag_area_len(r):
    body = bw.encode_record(r)[0][4:]
    import grammarcases as G
    return len(body) - G.tag_area(body)


KIND_BYTES = {k: tag_area_len(_read("x", 0, xv=k)) - 6 for k in KINDS}


def records(deep=False, long_name=False):
    """the corpus' reads, unsorted.  `deep`: N_DEEP more reads in the main unit (it takes the deep tier of the walk);
    `long_name`: a read of a 129-byte name in the small unit (outside the walk's envelope: the host reader's unit)"""
    at = A0 - 50                 # a 100M read from here covers A0 +- 20: an is_ref_seq hit
    out = []
    # tag areas of every length a well-formed area with RG can have up to 72 bytes -- 6 (RG alone), then 10 and up: a field takes at
    # least four bytes --, each on a read that is tagged (a hit: its area is rewritten) and on a mate that is not hit (its area is
    # copied whole unless the pair's verdict sets it); the XV kinds in turn, an XP:Z of the right size making up the length
    for i, want in enumerate(AREAS):
        name = "t%02d" % i + "x" * (i % 5)
        kind = KINDS[want % 7]
        rest = want - 6 - KIND_BYTES[kind]
        if rest < 0 or 0 < rest < 4:
            kind, rest = "none", want - 6
        out.append(_read(name, at + i % 25, 0x41, xv=kind, pad=rest - 4 if rest else None))
        out.append(_read(name, at + 420 + i % 7, 0x81 | 0x10, xv=KINDS[(i + 3) % 7], pad=None if i % 3 else i % 11))
    out.append(_read("only_xv_and_rg", at, 0x41, xv="only_besides_rg"))
    # a pair that straddles the deletion: the verdict's tag_span branches
    for i in range(6):
        out.append(_read("pair%d" % i, A0 - 100 - 10 * i, 0x41, xv=KINDS[i]))
        out.append(_read("pair%d" % i, B0 + 30 + 5 * i, 0x81 | 0x10, xv=KINDS[(i + 1) % 7]))
    # three and four primaries (continuation rows): one hit each, the rest neither hit nor paired
    for n, name in ((3, "three"), (4, "four")):
        for j, flag in enumerate((0x41, 0x81, 0x51, 0x91)[:n]):
            out.append(_read(name, at + 5 if j == 1 else A0 - 400 + 30 * j, flag, xv="z_last" if j == 2 else "none"))
    # a hit with MAPQ 0
    out.append(_read("mapq0", at + 3, 0x41, mapq=0))
    out.append(_read("mapq0", B0 + 200, 0x81 | 0x10, mapq=0, xv="z_last"))
    # a seq candidate (SA) and a clip candidate (soft clip, no SA) in one fragment, both supporting the breakpoint
    out.append(_read("seq_and_clip", A0 - 60, 0x41, cigar="60M40S", extra=[("SA", "Z", SEQ_SA)], xv="z_first"))
    out.append(_read("seq_and_clip", A0 - 60, 0x81, cigar="60M40S", xv="twice"))
    # ... and fragments where only one of the two supports it: which read gets its A says which candidate is which (every read here
    # has an XV of its own, so tag_span sets none of them, and none is a hit: an A can only come from its own candidate's verdict bit)
    out.append(_read("seq_only", A0 - 60, 0x41, cigar="60M40S", extra=[("SA", "Z", SEQ_SA)], xv="z_last"))
    out.append(_read("seq_only", A0 - 200, 0x81, cigar="60M40S", xv="z_last"))
    out.append(_read("clip_only", A0 - 200, 0x41, cigar="60M40S", extra=[("SA", "Z", "1,60001,+,60S40M,60,0;")], xv="z_last"))
    out.append(_read("clip_only", A0 - 60, 0x81, cigar="60M40S", xv="z_last"))
    # fragments that write nothing: no hit, no pair, no candidate -- one of them with an XV of its own
    out.append(_read("silent", A0 - 420, 0x41))
    out.append(_read("silent_xv", A0 - 410, 0x41, xv="z_last"))
    # names of 1 and 128 bytes
    out.append(_read("n", at + 1, 0x41))
    out.append(_read("N" * 128, at + 2, 0x41, xv="a_type"))
    # a secondary alignment beside its primary: only its (name, flag) counts, it is never written
    out.append(_read("with_secondary", at + 4, 0x41))
    out.append(_read("with_secondary", at + 9, 0x141))
    # the small unit
    for i in range(5):
        out.append(_read("small%d" % i, 70_000 + i, 0x41, xv=KINDS[i]))
        out.append(_read("small%d" % i, 70_420 + i, 0x81 | 0x10, xv=KINDS[(i + 2) % 7]))
    if long_name:
        out.append(_read("L" * 129, 70_003, 0x41, xv="z_last"))
    if deep:
        for k in range(N_DEEP):
            out.append(_read("deep%04d" % ((k * 37) % N_DEEP), A0 - 440 + k % 60, 0x41 if k % 2 else 0x81, xv=KINDS[k % 7] if k % 9 == 0 else "none"))
    return out


SITES = ((10_000, "e0"), (A0, "d1"), (70_050, "d2"), (90_000, "e3"))


def write_case(tmp_path, name="dump", **kw):
    """(bam, vcf, library json) of the corpus for the drivers"""
    import test_host_pipeline as H
    path = WC.write_case(tmp_path, name, records(**kw))
    lib_json = str(tmp_path / (name + ".json"))
    with open(lib_json, "w") as f:
        json.dump(WC.INFO, f)
    header = [l for l in open(H.IN_VCF) if l.startswith("##")]
    body = ["1\t%d\t%s\tN\t<DEL>\t0\t.\tSVTYPE=DEL;SVLEN=-800;END=%d;STR=+-:10;CIPOS=0,0;CIEND=0,0\n" % (a, ident, a + 800) for a, ident in SITES]
    vcf = str(tmp_path / (name + ".vcf"))
    with open(vcf, "w") as f:
        f.write("".join(header) + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(body))
    return path, vcf, lib_json


def reach(written, source):
    """What the corpus has to reach, from the Python route's output (`written`: the bam.AlignedSegment records of the BAM it wrote)
    and the corpus' own records (`source`)."""
    by_name = {}
    for r in written:
        by_name.setdefault(r.query_name, []).append(r)
    src = {(r["name"], r["flag"]): r for r in source}
    kinds = {}                                     # XV kind of the input read -> the XV fields written for such reads
    for r in written:
        xv = [f for n, f in tag_fields_any(r._tagbytes) if n == b"XV"]
        kinds.setdefault(src[(r.query_name, r.flag)]["xv_kind"], set()).add(tuple(xv))
    assert len(by_name["three"]) == 3 and len(by_name["four"]) == 4
    assert set(kinds) == set(KINDS)                                                      # every XV kind was written
    set_a, set_r = (b"XVAA",), (b"XVAR",)
    assert all(kinds[k] & {set_a, set_r} for k in KINDS if k != "none")                  # ... replaced by one XV:A
    assert (b"XVZR\0",) in kinds["z_last"] and any(len(v) == 2 for v in kinds["twice"])   # ... and kept as it was where nothing set it
    assert any(r.mapping_quality == 0 and r.get_tag("XV") == "R" and r._tagbytes.endswith(b"XVAR") for r in by_name["mapq0"])
    assert [r._tagbytes[-4:] for r in by_name["seq_and_clip"]] == [b"XVAA", b"XVAA"]
    xv_of = lambda name: {bool(src[(r.query_name, r.flag)]["tags"][-1][0] == "SA"): [f for n, f in tag_fields_any(r._tagbytes) if n == b"XV"]
                          for r in by_name[name]}                 # {the read with the SA tag: its XV fields, the other: its}
    assert xv_of("seq_only") == {True: [b"XVAA"], False: [b"XVZR\0"]}       # verdict bit 16 alone: A on the read behind the seq candidate
    assert xv_of("clip_only") == {True: [b"XVZR\0"], False: [b"XVAA"]}      # verdict bit 32 alone: A on the read behind the clip candidate
    assert "silent" not in by_name and "silent_xv" not in by_name and all(not r.flag & 0x100 for r in written)
    assert len(by_name["n"]) == 1 and len(by_name["N" * 128]) == 1
    assert any(not r.has_tag("XV") for r in written)                                     # a read nothing set, without an XV of its own
    lens = {len(src[(r.query_name, r.flag)]["name"]) for r in written}
    areas = {tag_area_len(src[(r.query_name, r.flag)]) for r in written if r._tagbytes.endswith((b"XVAR", b"XVAA"))}
    assert {1, 128} <= lens and set(AREAS) <= areas, sorted(set(AREAS) - areas)
    return by_name


def tag_fields_any(b):
    """[(name, the field's bytes)] of a well-formed tag area, B arrays included"""
    import struct
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    out, i = [], 0
    while i < len(b):
        t = chr(b[i + 2])
        if t in "ZH":
            j = b.index(b"\0", i + 3) + 1
        elif t == "B":
            j = i + 8 + struct.unpack_from("<I", b, i + 4)[0] * size[chr(b[i + 3])]
        else:
            j = i + 3 + size[t]
        out.append((b[i:i + 2], b[i:j]))
        i = j
    return out

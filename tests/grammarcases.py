"""Inputs shared by tests/test_record_grammar_host.py (CPU) and tests/test_record_grammar_device.py (GPU): a corpus of tag areas
that holds every BAM tag type, every B subtype and payloads that spell a tag inside another tag's value, as decorations of the
reads of one known DEL site (walkcases.HEADER / SITE / INFO), and a CIGAR list for the operation classes.  The reference of the
tag grammar is spec_tags below: the type table of the SAM specification (section 4.2.4) restated with `struct` alone.

A decoration is (label, tags): a tag list in which the markers RG_HERE and SA_HERE stand for the read's own RG:Z and SA:Z.  It
is applied to a plain 100M read (SA_HERE dropped) and to a split candidate (60M40S with REAL_SA)."""
import gzip
import struct

import bamwriter as bw
import libscancases as lc
import walkcases as W

RG_HERE, SA_HERE = "<RG>", "<SA>"
REAL_SA = "1,50852,+,60S40M,60,0;"          # the other piece of a 60M40S read that ends at breakend A, at breakend B
FAKE_SA = "2,777,-,30M70S,60,0;"            # a valid entry that is not the read's: taking it changes the records
SPELL_RG = b"RGZother\0"                    # ("other" is no read group of the header: taking it is unknown_rg)
SPELL_SA = b"SAZ" + FAKE_SA.encode() + b"\0"
SUBTYPES = "cCsSiIf"
COUNTS = (0, 1, 3, 17)
_RANGE = {"c": (-128, 127), "C": (0, 255), "s": (-32768, 32767), "S": (0, 65535), "i": (-2 ** 31, 2 ** 31 - 1), "I": (0, 2 ** 32 - 1)}


def _scalars(p, k):
    """every scalar type once under keys that begin with `p`; k = 0 / 1 / 2: the smallest values (and the empty Z and H), the
    largest, values whose bytes are letters"""
    pick = lambda t: (_RANGE[t][0], _RANGE[t][1], (ord("G") if t in "cC" else 0x5A47))[k]
    return [(p + "A", "A", "RSZ"[k]), (p + "c", "c", pick("c")), (p + "C", "C", pick("C")), (p + "s", "s", pick("s")),
            (p + "S", "S", pick("S")), (p + "i", "i", pick("i")), (p + "I", "I", pick("I")),
            (p + "f", "f", (-0.0, 3.4028234663852886e38, 1.5)[k]), (p + "Z", "Z", ("", "RG:Z:rg SA:Z:1,2,+,3M,4,5;", "text")[k]),
            (p + "H", "H", ("", "1AE301", "52475A")[k])]


def _arrays(p, n, order=SUBTYPES):
    """a B array of `n` elements of every subtype, the extremes of the type among them"""
    def values(sub):
        if sub == "f":
            return [(-1.5, 0.0, 2.25, 1e30, -0.0)[j % 5] for j in range(n)]
        lo, hi = _RANGE[sub]
        return [(lo, hi, 0x47, lo // 2, hi // 2)[j % 5] for j in range(n)]
    return [(p + sub, "B", (sub, values(sub))) for sub in order]


def _raw_array(key, sub, size, payload):
    """a B array whose bytes are `payload`, padded with NULs to whole elements"""
    payload += b"\0" * (-len(payload) % size)
    return (key, "raw", key.encode() + b"B" + sub.encode() + struct.pack("<I", len(payload) // size) + payload)


def _spelled(p):
    """payloads that spell a tag: a walk that skips a byte too few or too many in front of or inside them lands on RGZother
    or on the fake SA entry"""
    rgzx_f, = struct.unpack("<f", b"RGZx")
    rgzx_i, = struct.unpack("<I", b"RGZx")
    return [(p + "1", "B", ("C", list(SPELL_RG))), (p + "2", "B", ("C", list(SPELL_SA))),
            _raw_array(p + "3", "I", 4, SPELL_RG + SPELL_SA), _raw_array(p + "4", "f", 4, SPELL_SA + SPELL_RG),
            (p + "5", "Z", "xRGZother SAZ" + FAKE_SA + " yRGZrg"), (p + "6", "f", rgzx_f), (p + "7", "I", rgzx_i),
            (p + "8", "Z", "")]              # (the NUL that ends "RGZx..." for a walk that landed on it)


_WRONG_RG = [("RG", "H", "6F74686572"), ("RG", "A", "o"), ("RG", "i", 0x5A4752)]
_WRONG_SA = [("SA", "H", "2C3737372C")]


def _everything(p):
    """all of the above under keys that begin with `p` (and, the empty arrays, with its capital)"""
    return (_scalars(p, 0)[:5] + _arrays(p, 3) + _scalars(p, 1)[5:] + _spelled(p) + _WRONG_RG + _WRONG_SA
            + _arrays(p.upper(), 0) + [("SA", "Z", FAKE_SA)])


CORPUS = [
    ("scalars_front", _scalars("a", 0) + [RG_HERE] + [SA_HERE]),
    ("scalars_between", [RG_HERE] + _scalars("b", 1) + [SA_HERE]),
    ("scalars_behind", [RG_HERE, SA_HERE] + _scalars("c", 2)),
    ("scalars_everywhere", _scalars("a", 2) + [RG_HERE] + _scalars("b", 0) + [SA_HERE] + _scalars("c", 1)),
    ("arrays0_front", _arrays("d", 0) + [RG_HERE, SA_HERE]),
    ("arrays1_between", [RG_HERE] + _arrays("e", 1) + [SA_HERE]),
    ("arrays3_front", _arrays("f", 3) + [RG_HERE, SA_HERE] + _arrays("g", 1, "fIiSsCc")),
    ("arrays17_between", [RG_HERE] + _arrays("h", 17) + [SA_HERE]),
    ("arrays17_last", [RG_HERE, SA_HERE] + _arrays("i", 0) + _arrays("j", 17, "fIiCcSs")),     # the record ends with a B:s array
    ("spell_rg_in_bytes", [("k1", "B", ("C", list(SPELL_RG))), RG_HERE, SA_HERE]),
    ("spell_sa_in_bytes", [RG_HERE, ("k2", "B", ("C", list(SPELL_SA))), SA_HERE]),
    ("spell_in_words", [_raw_array("k3", "I", 4, SPELL_RG + SPELL_SA), RG_HERE, SA_HERE]),
    ("spell_in_floats", [_raw_array("k4", "f", 4, SPELL_SA + SPELL_RG), RG_HERE, SA_HERE]),
    ("spell_in_text", [("k5", "Z", "xRGZother SAZ" + FAKE_SA + " yRGZrg"), RG_HERE, ("k6", "Z", "SAZ" + FAKE_SA), SA_HERE]),
    ("spell_in_scalars", _spelled("l")[5:] + [RG_HERE] + _spelled("m")[5:] + [SA_HERE]),
    ("wrong_type_rg", _WRONG_RG + [RG_HERE, SA_HERE]),
    ("wrong_type_sa", [RG_HERE] + _WRONG_SA + [SA_HERE]),
    ("second_rg_and_sa", [RG_HERE, SA_HERE, ("RG", "Z", "other"), ("SA", "Z", FAKE_SA)]),
    ("sa_first_all_between", [SA_HERE] + _everything("n") + [RG_HERE] + _scalars("o", 2)),
    ("rg_last_all_between", [SA_HERE] + _everything("p") + [RG_HERE]),
]

# one read per string over breakend A (50 050): (CIGAR, position, SA or None)
CIGARS = [("100M", 49_980, None), ("50=2X48=", 49_981, None), ("40M5P60M", 49_982, None), ("30M500N70M", 49_520, None),
          ("5H10S85M", 49_983, None), ("85M10S5H", 49_984, None), ("5H95M", 49_985, None), ("20M3I10M4D67M", 49_986, None),
          ("10S30M5D30M5I20M5S", 49_987, None), ("60M40H", 49_990, REAL_SA)]

# outside the envelope of the walk and of the Python reader: a B array of a subtype the specification does not have
UNKNOWN_SUBTYPE = ("XB", "raw", b"XBBd" + struct.pack("<I", 1) + b"\0" * 4)     # (a walk that takes 4 bytes per element passes)


def tags_of(decoration, rg, sa):
    """the decoration's tag list with the read's own RG (and SA, unless `sa` is None) in the places of the markers"""
    out = []
    for t in decoration:
        if t == RG_HERE:
            out.append(("RG", "Z", rg))
        elif t == SA_HERE:
            if sa is not None:
                out.append(("SA", "Z", sa))
        else:
            out.append(t)
    return out


def decorated(k, prefix=""):
    """the two reads of decoration k: the plain one over breakend A and the split candidate that ends on it"""
    label, deco = CORPUS[k % len(CORPUS)]
    plain = W._read("%sp%02d_%s" % (prefix, k, label), 49_955 + k % len(CORPUS), tags=tags_of(deco, "rg", None))
    split = W._read("%ss%02d_%s" % (prefix, k, label), 49_990, cigar="60M40S", tags=tags_of(deco, "rg", REAL_SA))
    return plain, split


def cigar_reads():
    return [W._read("c%02d" % k, pos, cigar=cigar, tags=[("RG", "Z", "rg")] + ([("SA", "Z", sa)] if sa else []))
            for k, (cigar, pos, sa) in enumerate(CIGARS)]


def evidence_records():
    return [r for k in range(len(CORPUS)) for r in decorated(k)] + cigar_reads()


def _open(tmp_path, name, records):
    sample, nbam = W.open_sample(W.write_case(tmp_path, name, records), W.INFO)
    return [{"breakpoint": W.SITE}], sample, nbam


def evidence_input(tmp_path, records=None, name="grammar"):
    """the decorated reads and the CIGAR list at SITE: one unit of fewer than 64 kept reads"""
    return _open(tmp_path, name, evidence_records() if records is None else records)


N_DEEP = 1100


def deep_records():
    """the decorations cycled over N_DEEP reads of different names (plain and split in turn): more kept reads than the on-chip
    tier holds (deepcases.LDS), so the deep kernel walks the unit"""
    out = []
    for k in range(N_DEEP // 2):
        plain, split = decorated(k, prefix="d%03d" % k)
        out += [plain, dict(split, flag=0x1 | 0x80)]
    return out


def deep_input(tmp_path):
    return _open(tmp_path, "grammar_deep", deep_records())


N_LIBRARY = 400
_LONG_CIGARS = ["1000M", "50S950M", "400M20I580M", "300M50D700M", "1001M", "200=30X770M100S", "600M400H", "*"]


def library_records():
    """libscancases.synthetic_records in small, with a decoration's tags in front of RG (the library walk stops at RG) and reads
    long enough that the file takes more than one round of libscancases.SMALL_ROUND"""
    recs = lc.synthetic_records(4, n=N_LIBRARY)
    for i, r in enumerate(recs[:N_LIBRARY]):
        rg = dict((key, val) for key, _typ, val in r["tags"])["RG"]
        _label, deco = CORPUS[i % len(CORPUS)]
        r["tags"] = tags_of(deco[:deco.index(RG_HERE) + 1], rg, REAL_SA) + [("XS", "i", 5)]
        r["cigar"] = _LONG_CIGARS[i % len(_LONG_CIGARS)]
    return recs


def library_input(path):
    bw.write_bam(path, lc.HEADER, lc.REFS, library_records(), block_bytes=3000)
    return path


# ---- the reference: the tag grammar from the SAM specification's table, nothing of svtyper_amd --------------------------------
_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def tag_area(record):
    """where the tags of a record begin (`record`: the bytes behind block_size)"""
    l_name, n_cigar, l_seq = record[8], struct.unpack_from("<H", record, 12)[0], struct.unpack_from("<i", record, 16)[0]
    return 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def walk_spec(record, at):
    """(key, type, offset of the value, its length in bytes) of every tag from `at` on; for Z and H the length without the NUL,
    for B with its 5-byte header"""
    while at < len(record):
        key, typ = record[at:at + 2].decode("ascii"), chr(record[at + 2])
        at += 3
        if typ in _SIZE:
            size = _SIZE[typ]
        elif typ in "ZH":
            size = record.index(b"\0", at) - at
        elif typ == "B":
            size = 5 + _SIZE[chr(record[at])] * struct.unpack_from("<I", record, at + 1)[0]
        else:
            raise ValueError("type %r" % typ)
        if at + size + (typ in "ZH") > len(record):
            raise ValueError("tag %s runs over the record" % key)
        yield key, typ, at, size
        at += size + (typ in "ZH")


def spec_tags(record):
    """(the first RG:Z value or None, the first SA:Z value or None) of a record"""
    found = {}
    for key, typ, at, size in walk_spec(record, tag_area(record)):
        if typ == "Z" and key in ("RG", "SA") and key not in found:
            found[key] = record[at:at + size].decode("ascii")
    return found.get("RG"), found.get("SA")


def iter_records(path):
    """the alignment records of a BAM file, each without its block_size"""
    with gzip.open(path, "rb") as f:
        data = f.read()
    at = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref, = struct.unpack_from("<i", data, at)
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", data, at)[0]
    while at < len(data):
        size, = struct.unpack_from("<i", data, at)
        yield data[at + 4:at + 4 + size]
        at += 4 + size


def type_census(path):
    """the tag type codes of a file ("B:" + subtype for arrays) with the number of tags of each"""
    seen = {}
    for rec in iter_records(path):
        for _key, typ, at, _size in walk_spec(rec, tag_area(rec)):
            code = typ if typ != "B" else "B:" + chr(rec[at])
            seen[code] = seen.get(code, 0) + 1
    return seen

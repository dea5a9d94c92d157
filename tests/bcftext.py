"""A decoded BCF record (a dict of tests/bcfreader.py: read_record) as the VCF data line the decoder is held to, in plain Python from
the issue's wording of the line format: what `bcftools view` is understood to print.  Nothing here imports svtyper_amd.

Floats print by Python's '%g' of the float32 widened to double (C's %g: six significant digits, trailing zeros stripped, exponent
form below 1e-4 and from 1e6); a nan prints 'nan' whatever its sign.  `in_envelope` restates, from the stated envelope and in exact
rational arithmetic, which floats the shared rule formats itself: zero of either sign, or 1e-4 <= |x| < 1e6."""
from fractions import Fraction

import numpy as np


def float_of(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def float_text(bits):
    x = float_of(bits)
    return "nan" if x != x else "%g" % x


def in_envelope(bits):
    x = float_of(bits)
    if x != x or x in (float("inf"), float("-inf")):
        return False
    return x == 0 or Fraction(1, 10000) <= abs(Fraction(x)) < 1000000


def _numbers(values, text):
    return ",".join("." if v is None else text(v) for v in values) if values else "."


def _gt(values):
    out = ""
    for i, (allele, phased) in enumerate(values):
        out += ("|" if phased else "/") if i else ""
        out += "." if allele is None else str(allele)
    return out or "."


def _value(value, declared):
    if declared == "Integer":
        return _numbers(value, str)
    if declared == "Float":
        return _numbers(value, float_text)
    return value


def record_floats(rec, d):
    """the float32 bit patterns of the record that are values: QUAL and what its Float keys hold"""
    bits = [] if rec["qual"] is None else [rec["qual"]]
    for key, value in rec["info"]:
        if value is not True and d["types"][("INFO", key)] == "Float":
            bits += [v for v in value if v is not None]
    for row in rec["samples"]:
        for key, value in zip(rec["format"], row):
            if key != "GT" and d["types"][("FORMAT", key)] == "Float":
                bits += [v for v in value if v is not None]
    return bits


def line(rec, d):
    """the data line of `rec`, its newline included; `d`: the dictionaries of bcfreader.read_header (the Type a key's values were
    read by: the reader holds Integer and Float vectors both as lists of ints)"""
    cols = [rec["chrom"], str(rec["pos"]), rec["id"] or ".", rec["ref"], ",".join(rec["alt"]) or ".",
            "." if rec["qual"] is None else float_text(rec["qual"]), "." if not rec["filter"] else ";".join(rec["filter"])]
    info = [key if value is True else "%s=%s" % (key, _value(value, d["types"][("INFO", key)])) for key, value in rec["info"]]
    cols.append(";".join(info) or ".")
    if rec["format"]:
        cols.append(":".join(rec["format"]))
        for row in rec["samples"]:
            parts = []
            for key, value in zip(rec["format"], row):
                if key == "GT":
                    parts.append(_gt(value))
                elif d["types"][("FORMAT", key)] in ("Integer", "Float"):
                    parts.append(_value(value, d["types"][("FORMAT", key)]))
                else:
                    parts.append(value or ".")
            cols.append(":".join(parts))
    return "\t".join(cols) + "\n"


def text(stream, R):
    """the VCF text of the BCF `stream` by the reader module `R` (tests/bcfreader.py): the header text, then the lines"""
    head, d, records, _offsets = R.read_bcf(stream)
    return head + "".join(line(rec, d) for rec in records), d, records

"""`python -m svtyper_amd.bcf_in`: a BCF2.2 file (BGZF) as VCF text -- what every program here reads.

    open_text(path_or_file, engine="host", device=0, block_bytes=None, stats=None) -> a binary file of lines
    is_bcf(path_or_file) -> bool
    python -m svtyper_amd.bcf_in in.bcf [-o out.vcf] [--engine host|device] [--device N] [--bgzf --sort --tabix ...]

The BGZF members are inflated on the host by the library's member code, every CRC-32 checked; the stream's header and record
chain are read on the host; the records become lines in the native library (include/svtyper_bcf.h: svt_bcf_text_host, or
svt_bcf_text_device -- one wavefront per record, lanes over samples; the same text, byte for byte) in chunks of at most
`block_bytes` of stream (None: cohort.BLOCK_BYTES["device"], on either engine).  The text is the header without its ,IDX=n attributes, then one line
per record in the format of DESIGN 3.4: what `bcftools view` is understood to print; byte equality with htslib is not claimed,
nothing here has htslib.  The CLI stands where `bcftools view` stood between the cohort steps; with the output options of the
other programs, `--bgzf --sort --tabix -o x.vcf.gz` converts a BCF in one run.

Nothing is repaired: BcfInputError names the file, the 1-based record and the kind (native_reads.BCF_TEXT_KINDS; "bgzf" and
"header" for a file that is no BGZF of a BCF stream)."""
from __future__ import annotations

import argparse
import io
import sys
import zlib
from typing import Optional

import numpy as np

from . import hip
from . import native_reads as nr
from .cohort import BLOCK_BYTES, _text, add_program_arguments, parse_program_arguments, run_program

MAGIC = b"BCF\2\2"
_WHAT = {"truncated": "the record runs out of the stream, or its l_shared is below 24",
         "index": "a contig, FILTER, INFO or FORMAT index the header's dictionaries do not hold",
         "samples": "an n_sample that is not the header's sample count",
         "type": "a type code that is none of 0, 1, 2, 3, 5, 7, or one its field cannot have",
         "count": "a long count that is no single integer, or a vector that runs beyond its part",
         "gt": "a GT that is not held in an integer type",
         "length": "a shared or individual part whose walk does not end at its length"}


class BcfInputError(ValueError):
    """the file cannot be read as BCF: `file` names it, `record` is the 1-based number of the record in the way (None: the file's
    frame) and `kind` says what is wrong with it"""

    def __init__(self, message, file=None, record=None, kind=None):
        super().__init__(message)
        self.file, self.record, self.kind = file, record, kind


def _first_payload(head: bytes, n: int) -> bytes:
    """the first `n` bytes of the first BGZF member's payload, b"" where `head` does not begin with one"""
    if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04":
        return b""
    xlen = head[10] | head[11] << 8
    extra = head[12:12 + xlen]
    at = 0
    while at + 4 <= len(extra) and extra[at:at + 2] != b"BC":
        at += 4 + (extra[at + 2] | extra[at + 3] << 8)
    if at + 6 > len(extra):
        return b""
    try:
        return zlib.decompressobj(-15).decompress(head[12 + xlen:], n)
    except zlib.error:
        return b""


def is_bcf(path_or_file) -> bool:
    """whether the file is BGZF whose first member's payload begins with the BCF2.2 magic.  A path is opened and closed; an open
    binary file must be able to peek (what it holds stays unread)"""
    if isinstance(path_or_file, (str, bytes)):
        with open(path_or_file, "rb") as f:
            head = f.read(1 << 16)
    elif hasattr(path_or_file, "peek"):
        head = path_or_file.peek(1 << 16)
    else:
        return False
    return _first_payload(bytes(head), len(MAGIC)) == MAGIC


def _inflate(name: str, data: bytes) -> bytes:
    block_off, out_off = nr.bgzf_members(data)
    end = 0
    if len(block_off):
        last = int(block_off[-1])
        xlen = data[last + 10] | data[last + 11] << 8
        extra, at = data[last + 12:last + 12 + xlen], 0
        while extra[at:at + 2] != b"BC":
            at += 4 + (extra[at + 2] | extra[at + 3] << 8)
        end = last + (extra[at + 4] | extra[at + 5] << 8) + 1
    if end != len(data) or not len(block_off):
        raise BcfInputError("%s: bytes at %d that are no BGZF member" % (name, end), name, None, "bgzf")
    try:
        stream, status = nr.bgzf_inflate(data, block_off, out_off, verified=True)
    except hip.SvtyperHipError as e:
        raise BcfInputError("%s: %s" % (name, e), name, None, "bgzf")
    bad = np.flatnonzero(status)
    if len(bad):
        raise BcfInputError("%s: BGZF member %d at byte %d: %s" % (name, bad[0] + 1, int(block_off[bad[0]]),
                                                                   nr.INFLATE_REASONS.get(int(status[bad[0]]), "does not inflate")), name, None, "bgzf")
    return stream.tobytes()


def decode(name: str, data: bytes, engine="host", device=0, block_bytes=None, stats: Optional[dict] = None) -> bytes:
    """the VCF text of the BCF file `data` (its BGZF bytes); `name` is what errors call it"""
    if engine not in ("host", "device"):
        raise ValueError("engine is 'host' or 'device'")
    if block_bytes is None:
        block_bytes = BLOCK_BYTES["device"]
    if block_bytes < 1:
        raise ValueError("block_bytes is at least 1")
    stream = _inflate(name, data)
    try:
        got = nr.bcf_text(stream, device if engine == "device" else None, block_bytes)
    except hip.SvtyperHipError as e:
        if "svt_bcf_text: " not in str(e):
            raise
        raise BcfInputError("%s: %s" % (name, str(e).split("svt_bcf_text: ", 1)[1]), name, None, "header")
    if got["bad_record"]:
        kind = nr.BCF_TEXT_KINDS.get(got["bad_kind"], str(got["bad_kind"]))
        raise BcfInputError("%s, record %d: %s" % (name, got["bad_record"], _WHAT.get(kind, kind)), name, got["bad_record"], kind)
    if stats is not None:
        stats.update(records=got["n_records"], chunks=got["chunks"], host_lines=got["host_lines"],
                     times=nr.bcf_text_last_times() if engine == "device" else {})
    return got["text"].tobytes()


def open_text(path_or_file, engine="host", device=0, block_bytes=None, stats: Optional[dict] = None):
    """`path_or_file` (a path, or an open binary file, which is read to its end and not closed) as a binary file of VCF lines: the
    header lines, then the body lines.  `stats`, a dict, receives records, chunks, host_lines (the records the host twin wrote for
    a float outside the device's envelope) and, for engine="device", times (native_reads.bcf_text_last_times)."""
    if isinstance(path_or_file, (str, bytes)):
        name = path_or_file if isinstance(path_or_file, str) else path_or_file.decode()
        with open(name, "rb") as f:
            data = f.read()
    else:
        name = str(getattr(path_or_file, "name", path_or_file))
        data = getattr(path_or_file, "buffer", path_or_file).read()
    out = io.BytesIO(decode(name, data, engine, device, block_bytes, stats))
    out.name = name
    return out


# ------------------------------------------------------------------------------------------ CLI
def get_args(argv=None):
    p = argparse.ArgumentParser(prog="svtyper-bcf-in", formatter_class=argparse.RawTextHelpFormatter, description=(
        "svtyper-bcf-in\ndescription: Write a BCF file as VCF text"))
    p.add_argument(metavar="bcf", dest="bcf_in", nargs="?", type=str, default=None, help="BCF input (default: stdin)")
    add_program_arguments(p, "where the records become lines: the native host code or the GPU (same output bytes) [host]", keep_contigs_help=None)
    return parse_program_arguments(p, argv, "bcf_in")


def main(argv=None):
    args = get_args(argv)
    try:
        f = open_text(args.bcf_in if args.bcf_in is not None else sys.stdin.buffer, engine=args.engine, device=args.device)
    except (BcfInputError, OSError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    return run_program(args, (), lambda out: out.write(_text(f.getvalue())))     # (the input's errors are all met: none is caught here)


def cli():
    from .driver import run_cli
    run_cli(main)


if __name__ == "__main__":
    cli()

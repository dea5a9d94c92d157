"""Output as BCF (`--bcf`: BCF2.2 in BGZF, what bcftools merge / concat / view -r read fastest; with `sort=True, index="csi"` one
they can query by region): a text file-like object that sv_genotype and sso_genotype take as their `vcf_out` unchanged.

    out = open_bcf("calls.bcf", deflate="device", sort=True, index="csi")
    sso_genotype(bam, vcf_in, out, ...)
    out.close()                                  # the records, the members, the EOF member, calls.bcf.csi

The writer always holds the whole VCF text until close(): the header, which the drivers finish before their first record, is
the dictionary every record is encoded against.  close() works on the text as one piece -- the header's dictionaries (PASS,
then the FILTER / INFO / FORMAT IDs in order of first appearance; the ##contig IDs), with `sort` the body in the stable order by
(contig rank, POS) that `--bgzf --sort` writes, one BCF record per data line (svtyper_amd/csrc/svt_bcf.h: the record rule, one
piece of source for the host and the GPU), the stream cut into members every 65 280 bytes, and with `index` the `.csi` beside
them, folded from the records' spans by the fold of the `-w` BAM's index.  With deflate="device" the text goes to the GPU once
and the line table, the records and the members are made there (svt_bcf_bgzf_device) and the index is folded there; otherwise
on the host, by the same source.  The header text inside the BCF is the text the VCF route writes, byte for byte.

Nothing is repaired: a line the header does not cover, or a token that is none of its declared Type, raises BcfError with the
line's number and the key in the way, and the file is left as the BGZF writers leave theirs -- complete as BGZF, without records."""
from __future__ import annotations

import io
import os

import numpy as np

from .bgzf import PAYLOAD, BgzfWriter, close_held

_WHY = {"columns": "is not a VCF data line (8 tab-separated columns)", "contig": "names a contig that is no ##contig of the header",
        "pos": "has a POS that is no number below 2^31 - 1", "filter": "has a FILTER the header does not declare",
        "info_key": "has an INFO key the header does not declare", "format_key": "has a FORMAT key the header does not declare",
        "info_value": "has an INFO value that is none of its declared Type (or an integer outside int32's values)",
        "format_value": "has a sample value that is none of its declared Type (or an integer outside int32's values, or more fields than FORMAT)",
        "samples": "has a FORMAT column without samples, or a sample count that is not the header's", "qual": "has a QUAL that is no number"}
_NAMED = {"columns": None, "contig": "CHROM", "pos": "POS", "samples": "FORMAT", "qual": "QUAL"}


class BcfError(ValueError):
    """the text cannot be written as BCF as it is: `line` is the 1-based number of the line in the way, `kind` why (a value of
    native_reads.BCF_KINDS, or "order": an index was asked for and the records are not coordinate-sorted), `key` the key,
    FILTER name or column it is about"""

    def __init__(self, message: str, line: int, kind: str, key=None):
        super().__init__(message)
        self.line, self.kind, self.key = line, kind, key


class BcfWriter:
    """write / flush / close over a BgzfWriter: what sv_genotype and sso_genotype ask of their `vcf_out`"""

    def __init__(self, writer: BgzfWriter, name: str, sort: bool = False, index=None, index_path=None, stale=()):
        if index not in (None, "csi"):
            raise ValueError("index must be None or 'csi', not %r" % (index,))
        if index is not None and index_path is None:
            raise ValueError("index='csi' needs a path to write the index to: an output path, or index_path=")
        self._writer = writer
        self.name = name
        self.closed = False
        self._sort, self._index, self._index_path, self._stale = bool(sort), index, index_path, tuple(stale)
        self._held = []
        self.host_lines = 0         # after close(): lines whose floats lay outside the device's envelope (deflate="device")

    def write(self, text: str) -> int:
        if self.closed:
            raise ValueError("I/O operation on closed file")
        self._held.append(text.encode("utf-8"))
        return len(text)

    def writable(self) -> bool:
        return True

    def flush(self) -> None:
        """nothing: the text is written by close()"""

    def close(self) -> None:
        if not self.closed:
            self.closed = True
            self._close_held()

    def _close_held(self) -> None:
        """the held text as one piece: dictionaries, order, records, members, index -- what bgzf.close_held asks of its writer"""
        from . import native_reads as nr
        text = b"".join(self._held)
        self._held = []
        if text and not text.endswith(b"\n"):
            text += b"\n"

        def members(w):
            """-> the encoding call's result, member tables included where the device made the members"""
            if w._deflate == "device":
                made = nr.bcf_bgzf_device(text, self._sort, w._huffman, w._device)
            else:
                made = nr.bcf_encode(text, self._sort)
            if made["bad_line"]:
                raise self._refusal(text, made)
            self.host_lines = made["host_lines"]
            if w._deflate == "device":
                w._f.write(made["bytes"].tobytes())
            else:
                stream = made["bytes"].tobytes()
                for at in range(0, len(stream), PAYLOAD):
                    w.write(stream[at:at + PAYLOAD])
            return made

        def fold(made, log):
            return nr.csi_build_bam(made["spans"], made["n_ref"], made["l_ref_max"], np.array(log.starts, np.uint64), np.array(log.offsets, np.uint64),
                                    device=self._writer_device)

        def order_error(made, bad, kind):
            span = made["spans"][bad - 1]
            why = "lies in front of the record before it" if kind == nr.BAM_KIND_KEY_BACK else "cannot be held by the index's scheme"
            return BcfError("%s: record %d (contig %d, POS %d) %s: a .csi index needs coordinate-sorted records; no index was written -- "
                            "use --sort (sort=True)" % (self.name, bad, int(span["tid"]) + 1, int(span["beg"]) + 1, why), bad, "order")

        def write_as_bgzf(path, csi):
            index = BgzfWriter(path)
            index.write(csi)
            index.close()
        self._writer_device = self._writer._device if self._writer._deflate == "device" else None
        close_held(self._writer, self._index_path, members, self._index and fold, order_error, write_as_bgzf,
                   stale=self._stale if self._index else ())

    def _refusal(self, text: bytes, made: dict) -> BcfError:
        from . import native_reads as nr
        kind = nr.BCF_KINDS.get(made["bad_kind"], "columns")
        line = text.split(b"\n", made["bad_line"])[made["bad_line"] - 1]
        key = _NAMED.get(kind, "")
        if key == "":                                   # the key or name that begins at bad_at
            end = at = made["bad_at"]
            while end < len(line) and line[end:end + 1] not in (b"\t", b";", b"=", b":", b","):
                end += 1
            key = line[at:end].decode("utf-8", "replace")
        where = "line %d (%s)" % (made["bad_line"], line[:200].decode("utf-8", "replace").replace("\t", ":", 1).split("\t")[0])
        return BcfError("%s: %s %s%s; no record was written" % (self.name, where, _WHY[kind], ": %s" % key if key else ""), made["bad_line"], kind, key)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_bcf(file_or_path, deflate: str = "zlib", huffman: str = "fixed", device: int = 0, sort: bool = False, index=None, index_path=None,
             level: int = 6) -> BcfWriter:
    """`file_or_path`: a path, a binary file object, or a text file object over one (sys.stdout, what argparse.FileType("w")
    opens): its buffer is written to.  close() encodes, writes the EOF member and closes what was handed in.  `sort`,
    `index="csi"`: the module's docstring; the index goes to `index_path`, by default the output's path and ".csi" (a file object
    without a path of its own needs index_path=).  With `index` and without `sort`, records that are not coordinate-sorted make
    close() raise BcfError (kind "order") once the BCF is complete; no index is left behind.  An index of an earlier file
    beside the output is removed."""
    target = file_or_path
    if isinstance(target, io.TextIOBase) and hasattr(target, "buffer"):
        target.flush()
        target = target.buffer
    name = file_or_path if isinstance(file_or_path, str) else getattr(file_or_path, "name", "<bcf>")
    if index not in (None, "csi"):
        raise ValueError("index must be None or 'csi', not %r" % (index,))
    own = file_or_path if isinstance(file_or_path, (str, os.PathLike)) else getattr(file_or_path, "name", None)
    own = os.fspath(own) if isinstance(own, (str, os.PathLike)) and not str(own).startswith("<") else None
    stale = (own + ".csi",) if index is not None and own is not None else ()
    if index is not None and index_path is None:
        if own is None:
            raise ValueError("index='csi' needs a path to write the index to: an output path, or index_path=")
        index_path = own + ".csi"
    return BcfWriter(BgzfWriter(target, level=level, deflate=deflate, device=device, huffman=huffman), str(name), sort=sort, index=index,
                     index_path=index_path, stale=stale)

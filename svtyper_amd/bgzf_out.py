"""Text output as BGZF (`--bgzf`: a .vcf.gz that bcftools, tabix and IGV read as a stream; with `sort=True, index="tbi"` one they
can query by region): a text file-like object over bgzf.BgzfWriter.

    out = open_text("calls.vcf.gz", deflate="device")
    sso_genotype(bam, vcf_in, out, ...)
    out.close()                                  # the last member, the EOF member, and the file is closed

The members are cut every 65 280 bytes of UTF-8, wherever that falls; who compresses them is BgzfWriter's `deflate`, and
into which block its `huffman`.

`sort=True` (`--sort`) and `index="tbi"` (`--tabix`).  With either, nothing is written before close(): the writer keeps the
whole output text, which costs host memory equal to the output's size, and close() works on it as one piece -- its line table
(svtyper_amd/csrc/svt_vcf_lines.h: the per-line rule of the tabix VCF preset), with `sort` the lines in stable order by (contig
rank, POS, arrival) behind the header, the members, and with `index` the `.tbi` beside them.  A contig's rank is its place among
the header's ##contig lines, undeclared contigs follow in order of first appearance; BND mates, which the drivers write next
to each other, therefore part.  With deflate="device" the text goes to the GPU once and the table, the gather and the members
are made there (svt_vcf_bgzf_device); otherwise on the host, by the same source.  The index fold is host code either way
(svt_tbx_build; with `csi=True` -- `--csi` -- svt_csi_build_vcf: the same index as a `.csi`, which also holds lines that end
beyond 2^29).  Without either option the writer streams as it always did."""
from __future__ import annotations

import io
import os

from .bgzf import PAYLOAD, BgzfWriter, close_held


class VcfOrderError(ValueError):
    """the text cannot be sorted or indexed as it is: `line` is the 1-based number of the line in the way"""

    def __init__(self, message: str, line: int):
        super().__init__(message)
        self.line = line


class BgzfTextWriter:
    """write / flush / close over a BgzfWriter: what sv_genotype and sso_genotype ask of their `vcf_out`"""

    def __init__(self, writer: BgzfWriter, name: str, sort: bool = False, index=None, index_path=None, csi: bool = False, stale=()):
        if index not in (None, "tbi"):
            raise ValueError("index must be None or 'tbi', not %r" % (index,))
        if csi and index is None:
            raise ValueError("csi=True says which container the index goes into: it needs index='tbi'")
        if index is not None and index_path is None:
            raise ValueError("index='tbi' needs a path to write the index to: an output path, or index_path=")
        self._writer = writer
        self.name = name
        self.closed = False
        self._sort, self._index, self._index_path = bool(sort), index, index_path
        self._csi, self._stale = bool(csi), tuple(stale)
        self._held = [] if (sort or index) else None     # the whole text, until close()

    def write(self, text: str) -> int:
        if self.closed:
            raise ValueError("I/O operation on closed file")
        if self._held is not None:
            self._held.append(text.encode("utf-8"))
            return len(text)
        self._writer.write(text.encode("utf-8"))
        return len(text)

    def writable(self) -> bool:
        return True

    def flush(self) -> None:
        """what was written so far becomes members in the file (a flush cuts a member: not something to do per line)"""
        if self.closed or self._held is not None:       # (held text is written by close())
            return
        self._writer.flush()
        self._writer.drain()
        self._writer._f.flush()

    def close(self) -> None:
        if not self.closed:
            self.closed = True
            if self._held is None:
                self._writer.close()
            else:
                self._close_held()

    def _close_held(self) -> None:
        """the held text as one piece: line table, order, members, index -- what bgzf.close_held asks of its writer"""
        import numpy as np

        from . import native_reads as nr
        text = b"".join(self._held)
        self._held = []
        if self._sort and text and not text.endswith(b"\n"):
            text += b"\n"                               # (a last line that moves takes a newline with it)

        def members(w, text=text):
            """-> (a text, the table of the lines as written, where each lies in that text: None = where the table says)"""
            if w._deflate == "device":
                made, _off, lines, src_off, bad = nr.vcf_bgzf_device(text, self._sort, w._huffman, w._device)
                if bad:
                    raise self._order_error(text, nr.vcf_lines(text), bad, nr.TBX_NOT_DATA)
                w._f.write(made.tobytes())
                return text, lines, src_off
            lines = nr.vcf_lines(text)
            if self._sort:
                perm, bad = nr.vcf_sort_order(text, lines)
                if bad:
                    raise self._order_error(text, lines, bad, nr.TBX_NOT_DATA)
                text = nr.vcf_gather(text, lines, perm)
                lines = lines[perm]
                lines["off"] = np.cumsum(lines["len"]) - lines["len"]
            for at in range(0, len(text), PAYLOAD):
                w.write(text[at:at + PAYLOAD])
            return text, lines, None

        def order_error(held, bad, kind):
            text, lines, src_off = held
            if src_off is not None:
                lines = lines.copy()
                lines["off"] = src_off
            return self._order_error(text, lines, bad, kind)

        def write_as_bgzf(path, tbi):
            index = BgzfWriter(path)
            index.write(tbi)
            index.close()
        close_held(self._writer, self._index_path, members,
                   self._index and (lambda held, log: nr.tbx_build(held[0], held[1], np.array(log.offsets, np.uint64), held[2], csi=self._csi)),
                   order_error, write_as_bgzf, stale=self._stale if self._index else ())

    def _order_error(self, text, lines, bad, kind) -> VcfOrderError:
        """`lines`: a table whose `off` points into `text`"""
        from . import native_reads as nr
        line = lines[bad - 1]
        fields = text[int(line["off"]):int(line["off"]) + min(int(line["len"]), 200)].decode("utf-8", "replace").rstrip("\n").split("\t")
        where = "line %d (%s)" % (bad, ":".join(fields[:2]))
        if kind == nr.TBX_NOT_DATA:
            return VcfOrderError("%s: %s is not a VCF data line (8 tab-separated columns, POS a number below 2^31)" % (self.name, where), bad)
        if kind == nr.TBX_BEYOND and self._csi:
            return VcfOrderError("%s: %s ends beyond 2^32 - 2, the limit of the .csi index's scheme (min_shift 14, depth 6); no index "
                                 "was written" % (self.name, where), bad)
        if kind == nr.TBX_BEYOND:
            return VcfOrderError("%s: %s ends beyond 2^29, which a .tbi index cannot address (a CSI index is not written: ask for one "
                                 "with --csi (csi=True))" % (self.name, where), bad)
        why = "its contig reappears behind another one" if kind == nr.TBX_CONTIG_AGAIN else "its POS lies below the line in front"
        return VcfOrderError("%s: %s is out of order (%s): a %s index needs coordinate-sorted text; no index was written -- "
                             "use --sort (sort=True)" % (self.name, where, why, ".csi" if self._csi else ".tbi"), bad)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_text(file_or_path, deflate: str = "zlib", device: int = 0, level: int = 6, huffman: str = "fixed", sort: bool = False,
              index=None, index_path=None, csi: bool = False) -> BgzfTextWriter:
    """`file_or_path`: a path, a binary file object, or a text file object over one (sys.stdout, what argparse.FileType("w")
    opens): its buffer is written to.  close() writes the EOF member and closes what was handed in.  `sort`, `index="tbi"`: the
    module's docstring; the index goes to `index_path`, by default the output's path and ".tbi" (a file object without a
    path of its own needs index_path=).  With `index` and without `sort`, text that is not coordinate-sorted makes close()
    raise VcfOrderError once the .vcf.gz is complete; no index is left behind.  `csi=True` (`--csi`): the index asked for, in the
    CSI container (as pysam's tabix_index(..., csi=True) spells it) -- CSIv1 in the scheme (14, depth) whose depth is the smallest
    >= 5 that covers the largest end among the body lines, the tabix block as aux, at the output's path and ".csi"; it holds
    lines beyond 2^29.  `index="csi"` is not a spelling of it and `csi=True` without `index` is a ValueError.  An index of an
    earlier file beside the output is removed in either format, .tbi and .csi."""
    target = file_or_path
    if isinstance(target, io.TextIOBase) and hasattr(target, "buffer"):
        target.flush()
        target = target.buffer
    name = file_or_path if isinstance(file_or_path, str) else getattr(file_or_path, "name", "<bgzf>")
    if index not in (None, "tbi"):
        raise ValueError("index must be None or 'tbi', not %r" % (index,))
    if csi and index is None:
        raise ValueError("csi=True says which container the index goes into: it needs index='tbi'")
    stale = ()
    own = file_or_path if isinstance(file_or_path, (str, os.PathLike)) else getattr(file_or_path, "name", None)
    if index is not None and isinstance(own, (str, os.PathLike)) and not str(own).startswith("<"):
        stale = (os.fspath(own) + ".tbi", os.fspath(own) + ".csi")
    if index is not None and index_path is None:
        path = file_or_path if isinstance(file_or_path, (str, os.PathLike)) else getattr(file_or_path, "name", None)
        if isinstance(path, (str, os.PathLike)) and not str(path).startswith("<"):
            index_path = os.fspath(path) + (".csi" if csi else ".tbi")
        else:
            raise ValueError("index='tbi' needs a path to write the index to: an output path, or index_path=")
    return BgzfTextWriter(BgzfWriter(target, level=level, deflate=deflate, device=device, huffman=huffman), str(name), sort=sort,
                          index=index, index_path=index_path, csi=csi, stale=stale)

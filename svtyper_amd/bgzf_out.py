"""Text output as BGZF (`--bgzf`: a .vcf.gz that bcftools, tabix and IGV read): a text file-like object over bam.BgzfWriter.

    out = open_text("calls.vcf.gz", deflate="device")
    sso_genotype(bam, vcf_in, out, ...)
    out.close()                                  # the last member, the EOF member, and the file is closed

The members are cut every 65 280 bytes of UTF-8, wherever that falls; who compresses them is BgzfWriter's `deflate`, and
into which block its `huffman`."""
from __future__ import annotations

import io

from .bam import BgzfWriter


class BgzfTextWriter:
    """write / flush / close over a BgzfWriter: what sv_genotype and sso_genotype ask of their `vcf_out`"""

    def __init__(self, writer: BgzfWriter, name: str):
        self._writer = writer
        self.name = name
        self.closed = False

    def write(self, text: str) -> int:
        if self.closed:
            raise ValueError("I/O operation on closed file")
        self._writer.write(text.encode("utf-8"))
        return len(text)

    def writable(self) -> bool:
        return True

    def flush(self) -> None:
        """what was written so far becomes members in the file (a flush cuts a member: not something to do per line)"""
        if self.closed:
            return
        self._writer.flush()
        self._writer.drain()
        self._writer._f.flush()

    def close(self) -> None:
        if not self.closed:
            self.closed = True
            self._writer.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_text(file_or_path, deflate: str = "zlib", device: int = 0, level: int = 6, huffman: str = "fixed") -> BgzfTextWriter:
    """`file_or_path`: a path, a binary file object, or a text file object over one (sys.stdout, what argparse.FileType("w")
    opens): its buffer is written to.  close() writes the EOF member and closes what was handed in."""
    target = file_or_path
    if isinstance(target, io.TextIOBase) and hasattr(target, "buffer"):
        target.flush()
        target = target.buffer
    name = file_or_path if isinstance(file_or_path, str) else getattr(file_or_path, "name", "<bgzf>")
    return BgzfTextWriter(BgzfWriter(target, level=level, deflate=deflate, device=device, huffman=huffman), str(name))

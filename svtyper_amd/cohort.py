"""What the cohort programs that rewrite a VCF line by line share (svtyper_amd.classify, svtyper_amd.update_info): how an input is
opened, how its header is read and written again as the Vcf class of the reference's scripts does, and how its body is cut into
blocks for the native library, and what becomes of a block's records (finish_block).  The header's attributes themselves are
paste.py's (header_attributes, declared_lines)."""
from __future__ import annotations

import gzip
from typing import Iterable, Iterator, List, Optional, Tuple

GZIP_MAGIC = b"\x1f\x8b"


def open_source(source, sniff=False, engine="host", device=0):
    """(name, binary or text file, whether it is ours to close) of a path or an open file.  A path ending in .gz is read through
    gzip; `sniff`: so is whatever begins with the two bytes of a gzip member (an open file must be able to peek for that).  A BCF
    is read as its VCF text (bcf_in.open_text, decoded by `engine` on `device`): a path ending in .bcf, and with `sniff` whatever
    is BGZF whose payload begins with the BCF magic"""
    if isinstance(source, (str, bytes)):
        name = source if isinstance(source, str) else source.decode()
        zipped = name.endswith(".gz")
        bcf = name.endswith(".bcf")
        if sniff and not bcf:
            with open(name, "rb") as f:
                zipped = zipped or f.read(2) == GZIP_MAGIC
            bcf = zipped and _is_bcf(name)
        if bcf:
            return name, _bcf_text(name, engine, device), True
        return name, (gzip.open(name, "rb") if zipped else open(name, "rb")), True
    name = str(getattr(source, "name", source))
    if sniff and hasattr(source, "peek") and source.peek(2)[:2] == GZIP_MAGIC:
        if _is_bcf(source):
            return name, _bcf_text(source, engine, device), True
        return name, gzip.GzipFile(fileobj=source, mode="rb"), False
    return name, source, False


def _is_bcf(source):
    from . import bcf_in
    return bcf_in.is_bcf(source)


def _bcf_text(source, engine, device):
    from . import bcf_in
    return bcf_in.open_text(source, engine=engine, device=device)


def bytes_lines(f) -> Iterator[bytes]:
    for line in f:
        yield line.encode("utf-8", "surrogateescape") if isinstance(line, str) else line


def read_header(lines: Iterator[bytes]) -> Tuple[List[str], Optional[bytes]]:
    """(the lines in front of the first that does not begin with '#', that line or None)"""
    header = []
    for line in lines:
        if line[:1] != b"#":
            return header, line
        header.append(line.decode("utf-8", "surrogateescape"))
    return header, None


def chrom_lines(header: List[str]) -> List[str]:
    """the header's lines that begin with one '#' alone: the last of them names the samples"""
    return [h for h in header if h[1:2] != "#"]


def header_text(file_format, file_date, reference, declared: List[str], header: List[str], samples: List[str], keep_contigs, with_format=True):
    """the scripts' get_header: fileformat, fileDate, reference, the declared lines, the input's ##contig lines where they are
    kept, and the #CHROM line (`with_format`: its FORMAT column and the samples)"""
    columns = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"] + (["FORMAT"] + samples if with_format else [])
    return "\n".join(["##fileformat=" + file_format, "##fileDate=" + file_date, "##reference=" + reference] + declared
                     + ([h.rstrip("\n") for h in header if h.startswith("##contig")] if keep_contigs else []) + ["\t".join(columns)]) + "\n"


def blocks(first: bytes, lines: Iterable[bytes], block_bytes: int) -> Iterator[List[bytes]]:
    """the body from `first` on in lists of lines of at most `block_bytes` together, a line at the least"""
    block, size = [first], len(first)
    for line in lines:
        if size + len(line) <= block_bytes:
            block.append(line)
            size += len(line)
            continue
        yield block
        block, size = [line], len(line)
    yield block


def finish_block(name, done, block, text, samples, records, write, last_times, bad, vcf_out, stats, edit=None):
    """What follows a block's records in both programs: the lines in front of the one the script dies on are counted, joined again
    and written (write(text, results) -> out, out_off, report; edit(out, out_off, report, whole) -> out may change the text), the
    stats and the device's times are folded in, and the writer's report, then the records', is raised through bad(name, line, kind,
    text, sample).  `records`: (results, report) of the native call over `text`; `done`: the file's lines in front of the block"""
    results, info = records
    whole = info["bad_line"] - 1 if info["bad_line"] else len(block)
    if whole < len(block):
        text = b"".join(block[:whole])
    out, out_off, written = write(text, results[:whole])
    if written["bad_line"]:
        whole = written["bad_line"] - 1
    if edit is not None:
        out = edit(out, out_off, written, whole)
    vcf_out.write(out.decode("utf-8", "surrogateescape"))
    stats["lines"] += whole
    stats["blocks"] += 1
    for key in ("host_lines", "near_lines"):
        if key in info:
            stats[key] += info[key]
    stats["results"].append(results)
    if last_times is not None:
        for key, value in last_times().items():
            stats["times"][key] = stats["times"].get(key, 0.0) + value
    for report in (written, info):
        if report["bad_line"]:
            sample = samples[report["bad_sample"]] if report["bad_sample"] < len(samples) else None
            raise bad(name, done + whole + 1, report["bad_kind"], report["bad_text"], sample)

"""The blocks of tests/cohortlinecases.py on the host engine of svtyper_amd.classify and svtyper_amd.update_info, without a GPU: a
condition on those inputs before they go to one (tests/test_classify_device.py, tests/test_update_info_device.py).  Every line
is inside its rule's envelope (host_lines == 0, no mark), and every record is the one plain Python computes from the line's
tokens: the counts and the in-order sum of SQ for update_info; n_pos, the route and the DEL flag for classify."""
import functools

import numpy as np
import pytest

import cohortlinecases as K
from svtyper_amd import native_reads as nr

SLOPE, RSQUARED = 1.0, 0.2


@functools.lru_cache(maxsize=None)
def blocks(tool):
    return K.blocks(tool)


def run(tool, block, device=None):
    """(records, info, output text, the writer's info) of one block on the host (device None) or the device engine"""
    n = block["n_samples"]
    if tool == "classify":
        female = np.ones(n, np.uint8)
        records, info = nr.vcf_classify(block["text"], 1 - female, female, np.zeros(n, np.uint8), block["format_table"], SLOPE, RSQUARED,
                                        device=device)
        out, _off, written = nr.vcf_classify_write(block["text"], n, block["info_table"], block["format_table"], records)
    else:
        records, info = nr.vcf_update_info(block["text"], n, block["format_table"], device=device)
        out, _off, written = nr.vcf_update_info_write(block["text"], n, block["info_table"], block["format_table"], records)
    return records, info, out, written


EDGES = ("no text", "one line without its newline", "two lines")


@functools.lru_cache(maxsize=None)
def edges(tool):
    """the first block's lines in the shapes at the edges of a call: what its prologue (the upload, the line table) has the least of"""
    block = blocks(tool)[0]
    lines = block["text"].splitlines(True)
    return [dict(block, text=text) for text in (b"", lines[0][:-1], lines[0] + lines[1])]


@functools.lru_cache(maxsize=None)
def host(tool, k):
    """the host engine over block k, the edges counted on behind the blocks"""
    return run(tool, (blocks(tool) + edges(tool))[k])


def test_the_regions_cover_every_residue_and_length():
    for tool in ("classify", "update_info"):
        made = blocks(tool)
        assert [b["length"] for b in made] == [max(n, K.SHORTEST[tool]) for n in K.LENGTHS]
        assert any(b["last_piece_open"] for b in made)
        firsts, lasts = set(), set()
        for b in made:
            body = b["text"].split(b"\n")[:-1]
            assert sorted(l["offset"] % 16 for l in b["lines"]) == list(range(16)) and len(body) == 16
            for line, text, start in zip(b["lines"], body, np.cumsum([0] + [len(t) + 1 for t in body])):
                columns = text.split(b"\t")
                assert line["offset"] == start + len(b"\t".join(columns[:9])) + 1 and len(b"\t".join(columns[9:])) == b["length"]
                assert columns[0].decode() == line["chrom"] not in ("X", "Y") and len(columns) == 9 + b["n_samples"]
            firsts.add(b["lines"][0]["offset"] % 16)
            lasts.add(b["lines"][-1]["offset"] % 16)
        assert len(firsts) == len(lasts) == len(made) and not firsts & lasts
        assert max(b["n_samples"] for b in made) < 700 < nr.CLASSIFY_CAPACITY == nr.UPDATE_INFO_CAPACITY


@pytest.mark.parametrize("k", range(len(K.LENGTHS)))
def test_update_info_host_gives_the_plain_sums(k):
    block = blocks("update_info")[k]
    records, info, out, written = host("update_info", k)
    assert info["host_lines"] == 0 and info["bad_line"] == 0 and written["bad_line"] == 0 and len(records) == 16
    assert out.count(b"\n") == 16 and not records["flags"].any() and (records["route"] == nr.UPDATE_INFO_RULE).all()
    for rec, line in zip(records, block["lines"]):
        positive = [c for c in line["columns"] if c[0] not in ("0/0", "./.")]
        sum_sq = 0.0
        for c in positive:
            sum_sq += float(c[3])
        assert (rec["pe"], rec["sr"], rec["num_pos"]) == (sum(int(c[1]) for c in line["columns"]), sum(int(c[2]) for c in line["columns"]),
                                                          len(positive))
        assert rec["sum_sq"] == np.float64(sum_sq).view(np.uint64)


@pytest.mark.parametrize("k", range(len(K.LENGTHS)))
def test_classify_host_gives_the_plain_route(k):
    block = blocks("classify")[k]
    records, info, out, written = host("classify", k)
    assert info["host_lines"] == 0 and info["bad_line"] == 0 and written["bad_line"] == 0 and len(records) == 16
    assert out.count(b"\n") >= 16 and not (records["flags"] & nr.CLASSIFY_SLOW).any()
    for rec, line in zip(records, block["lines"]):
        n_pos = sum(c[0] not in ("./.", "0/0") for c in line["columns"])
        assert rec["n_pos"] == n_pos and rec["route"] == (nr.CLASSIFY_LOW if n_pos < 10 else nr.CLASSIFY_HIGH)
        assert bool(rec["flags"] & nr.CLASSIFY_DEL) == (line["svtype"] == "DEL")

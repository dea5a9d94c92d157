"""GPU: svtyper_amd.group_multiline with engine="device" (svtyper_amd/csrc/svt_vcf_group_kernel.h) over the corpus of
tests/groupcases.py: the golden bytes of the reference's script, the per-line records and the plan of the host engine byte for
byte, the number of lines the host's plain C++ decided (exactly the lines the corpus built for it), whether the join left the
device (exactly for the files that are not regular and the files with marked lines: a device path that hands everything over does
not pass), the deaths, the kernels' times, the regular files again with 4-bit hashes, and the command line into a sorted,
tabix-indexed BGZF file compressed on the device, read back by the independent reader of tests/tbxcases.py."""
import io
import os

import pytest

import groupcases as K
import tbxcases as X
import test_group_host as H
from svtyper_amd import cohort, group_multiline
from svtyper_amd import native_reads as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGULAR = [c for c in H.CASES if c["error"] is None and not c["irregular"] and not c["slow_lines"]]


@pytest.mark.parametrize("case", H.CASES, ids=[c["name"] for c in H.CASES])
def test_device_engine_gives_the_reference_bytes_and_the_hosts_plan(case, tmp_path, hip_device):
    golden = H.EXPECTED[case["name"]]["expected"]
    if case["error"] is not None:
        host = {}
        with pytest.raises(group_multiline.GroupError) as on_host:
            group_multiline.group_multiline(K.write_case(case, str(tmp_path)), vcf_out=io.StringIO(), file_date=H.GOLDEN["file_date"], stats=host)
        written, stats = io.StringIO(), {}
        with pytest.raises(group_multiline.GroupError) as e:
            group_multiline.group_multiline(K.write_case(case, str(tmp_path)), vcf_out=written, file_date=H.GOLDEN["file_date"], stats=stats,
                                            engine="device", device=hip_device)
        assert written.getvalue() == golden["stdout"]               # the lines in front of the one the script dies on
        assert (e.value.line, e.value.reference, e.value.verbatim, str(e.value)) == (on_host.value.line, on_host.value.reference,
                                                                                      on_host.value.verbatim, str(on_host.value))
        if case["kind"] is not None:
            assert stats["host_lines"] == case["slow_lines"] and stats["host_join"] == bool(case["slow_lines"])
            # the fatal cut: the records of every line, those at and behind the fatal one too, and the plan in front of it
            n_header = sum(l.startswith("#") for l in case["vcf"].splitlines())
            assert len(stats["records"]) == len(case["vcf"].splitlines()) - n_header
            assert stats["records"].tobytes() == host["records"].tobytes() and stats["plan"].tobytes() == host["plan"].tobytes()
            assert stats["lines"] == host["lines"] == case["error"] - n_header - 1 and stats["written"] == host["written"]
            times = stats["times"]
            assert times["lines_kernels_s"] > 0 and times["scan_kernel_s"] > 0 and times["compact_kernels_s"] > 0
        return
    _text, host = H.run(case, tmp_path)
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device)
    assert text == golden["stdout"]
    assert stats["host_lines"] == case["slow_lines"]                # exactly: nothing else is decided on the host
    assert stats["host_join"] == (case["irregular"] or case["slow_lines"] > 0)
    assert stats["records"].tobytes() == host["records"].tobytes() and stats["plan"].tobytes() == host["plan"].tobytes()
    assert stats["lines"] == host["lines"] and stats["written"] == host["written"]
    times = stats["times"]
    assert times["lines_kernels_s"] > 0 and times["scan_kernel_s"] > 0 and times["compact_kernels_s"] > 0
    n_bnd = int((stats["records"]["flags"] & 1).sum())
    if n_bnd and not case["slow_lines"]:
        assert times["match_kernel_s"] > 0
        if n_bnd >= 2 and not case["irregular"]:                    # (IDs that are all one ID need no radix pass)
            assert times["sort_kernels_s"] > 0
    if not stats["host_join"]:
        assert times["plan_kernels_s"] > 0


@pytest.mark.parametrize("case", REGULAR, ids=[c["name"] for c in REGULAR])
def test_four_bit_hashes_collide_and_the_bytes_decide(case, tmp_path, hip_device):
    _text, host = H.run(case, tmp_path)
    text, stats = H.run(case, tmp_path, engine="device", device=hip_device, hash_bits=4)
    assert text == H.EXPECTED[case["name"]]["expected"]["stdout"]
    assert stats["plan"].tobytes() == host["plan"].tobytes() and stats["records"].tobytes() == host["records"].tobytes()
    assert stats["host_join"] is False and stats["host_lines"] == 0


@pytest.mark.parametrize("shape", ["no text", "one line without its newline", "two lines"])
def test_the_edges_of_a_call_on_the_device(shape, hip_device):
    """what the call's prologue (the upload, the line table) has the least of, in the lines of last_line_bare, a pair: the host's
    records, plan, reports and text"""
    case = next(c for c in H.CASES if c["name"] == "last_line_bare")
    lines = [l.encode() for l in case["vcf"].splitlines(True)]
    header, body = [l.decode() for l in lines if l.startswith(b"#")], [l for l in lines if not l.startswith(b"#")]
    _ff, _ref, infos, _alts, formats, samples = group_multiline.header_tables(header)
    text = {"no text": b"", "one line without its newline": body[0][:-1], "two lines": body[0] + body[1] + b"\n"}[shape]
    tables = (len(samples), cohort.info_table(infos), cohort.format_table(formats))
    want = nr.vcf_group(text, tables[0], tables[2])
    got = nr.vcf_group(text, tables[0], tables[2], device=hip_device)
    assert len(got[0]) == text.count(b"\n") + (shape == "one line without its newline") and len(got[1]) == (2 if shape == "two lines" else 0)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[2] == dict(want[2], host_join=0) and want[2]["host_join"] == 1 and got[2]["bad_line"] == 0     # (where the join ran)
    wrote, asked = nr.vcf_group_write(text, *tables, got[0], got[1]), nr.vcf_group_write(text, *tables, want[0], want[1])
    assert wrote[0] == asked[0] and wrote[0].count(b"\n") == len(got[1]) and wrote[2] == asked[2] and wrote[2]["bad_line"] == 0


def test_the_regular_cases_are_most_of_the_corpus_and_hold_the_sizes():
    names = {c["name"] for c in REGULAR}
    assert names >= {"pairs_%d" % k for k in K.PAIR_COUNTS} | {"no_bnd", "unpaired_only", "id_lengths", "id_at_every_residue", "samples_0"}


def test_command_line_to_a_sorted_indexed_bgzf_file(tmp_path, hip_device):
    case = next(c for c in H.CASES if c["name"] == "pairs_257")
    out = str(tmp_path / "grouped.vcf.gz")
    r = H.command(case, tmp_path, ["--keep-contigs", "--engine", "device", "--device", str(hip_device), "--bgzf", "--sort", "--tabix", "--deflate",
                                   "device", "-o", out])
    assert r.returncode == 0, r.stderr
    kept, _s = H.run(case, tmp_path, keep_contigs=True)
    raw = open(out, "rb").read()
    members = X.Members(raw)
    assert H.dated(members.text().decode()).encode() == X.sorted_text(kept.encode())
    tbi = X.read_tbi(open(out + ".tbi", "rb").read())
    X.check_structure(raw, tbi, members)
    X.check_queries(raw, tbi, X.regions_of(members.text(), n_random=50), members)

"""The whole inflate="device" route with no GPU (svt_bam_evidence_walk_open_host): an arena laid out from BGZF headers alone,
inflated by the one-source decoder on the CPU, one open range per index chunk, and the walk ending every window where the fetch
does -- against the shipped host reader (svt_bam_evidence) and the host-inflate walk (svt_bam_evidence_walk_host)."""
import os
import struct
import zlib

import numpy as np
import pytest

import bamwriter as bw
import inflatecases as I
import walkcases as W
from svtyper_amd import hip, native_reads as nr

MODES = [(nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 120), (nr.COUNT_CLASSIC, 150)]


def _compare(sites, sample, nbam, mode, max_reads, flagged=None):
    a = W.unit_arrays(sites, sample, nbam, mode)
    want = nbam.evidence(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    got = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], max_reads, mode, a[4], 20, 3, 2)
    if flagged is None:
        assert not got[3].any(), "units flagged: %s" % {nr.WALK_REASONS[r] for r in got[3][got[3] != 0]}
        assert np.array_equal(got[0], want[0]), "record counts differ"
        assert got[1].tobytes() == want[1].tobytes(), "records differ"
        assert np.array_equal(got[2], want[2]), "skip flags differ"
    else:
        assert got[3].tolist() == flagged
        for u in range(len(sites)):
            if not flagged[u]:
                assert got[1][int(got[0][u]):int(got[0][u + 1])].tobytes() == want[1][int(want[0][u]):int(want[0][u + 1])].tobytes()
                assert got[2][u] == want[2][u]
    return want, got


@pytest.mark.parametrize("mode,max_reads", MODES)
def test_fixture_equals_the_host_reader(mode, max_reads):
    sites, sample, nbam = W.fixture_input()
    want, _ = _compare(sites, sample, nbam, mode, max_reads)
    assert len(want[1]) > 5000 or want[2].any()


@pytest.mark.parametrize("seed", W.SYNTHETIC_SEEDS)
def test_synthetic_bams_equal_the_host_reader(tmp_path, seed):
    sites, sample, nbam = W.synthetic_input(tmp_path, seed, tied_names=(seed % 2 == 0))
    for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_CLASSIC, 90), (nr.COUNT_SSO, 200)):
        _compare(sites, sample, nbam, mode, max_reads)


def test_fake_read_and_three_bam_inputs_equal_the_host_reader(tmp_path):
    for sites, sample, nbam in list(W.fake_inputs(tmp_path)) + list(W.three_bam_inputs(tmp_path)):
        for mode, max_reads in ((nr.COUNT_CLASSIC, None), (nr.COUNT_SSO, 1000), (nr.COUNT_SSO, 30), (nr.COUNT_CLASSIC, 25)):
            _compare(sites, sample, nbam, mode, max_reads)


@pytest.mark.parametrize("mode", [nr.COUNT_CLASSIC, nr.COUNT_SSO])
def test_max_reads_boundaries(tmp_path, mode):
    sites, sample, nbam = W.boundary_input(tmp_path, 37)
    for limit in (35, 36, 37, 38):
        want, _ = _compare(sites, sample, nbam, mode, limit)
        assert bool(want[2][0]) == (limit < (37 if mode == nr.COUNT_SSO else 36))


@pytest.mark.parametrize("case", ["reads", "name", "cigar", "sa_entries", "no_rg", "unknown_rg", "malformed_sa"])
def test_envelope_cases_flag_what_the_host_inflate_walk_flags(tmp_path, case):
    records, reason, _host_fails = W.envelope_cases(nr.walk_capacities())[case]
    sample, nbam = W.open_sample(W.write_case(tmp_path, case, records), W.INFO)
    a = W.unit_arrays([{"breakpoint": W.SITE}], sample, nbam, nr.COUNT_SSO)
    closed = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    opened = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert opened[3].tolist() == closed[3].tolist() and nr.WALK_REASONS[int(opened[3][0])] == reason


# ---- BAMs put together member by member: the corners of the open ranges --------------------------------------------------------
def _members_of(path):
    return I.file_members(path)


def _reindex(tmp_path, name, members, chunks, n_ref=2):
    """a BAM from `members` with a hand-written index: one bin (4681 + 3: positions 49 152 .. 65 535 of reference 0) holding
    `chunks`, linear index empty"""
    path = str(tmp_path / (name + ".bam"))
    with open(path, "wb") as f:
        f.write(b"".join(members))
    with open(path + ".bai", "wb") as f:
        f.write(b"BAI\x01" + struct.pack("<i", n_ref))
        f.write(struct.pack("<i", 1) + struct.pack("<Ii", 4681 + 3, len(chunks)))
        for beg, end in chunks:
            f.write(struct.pack("<QQ", beg, end))
        f.write(struct.pack("<i", 0))
        for _ in range(n_ref - 1):
            f.write(struct.pack("<ii", 0, 0))
    return path


def _corner_bam(tmp_path):
    """six reads in the window of W.SITE, two per data member, behind a member that holds the header alone (bamwriter cuts its
    stream anywhere; here every member starts with a record): (members, offsets of the members)"""
    refs = [("1", 100000), ("2", 100000)]
    text = W.HEADER.encode()
    head = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        head += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    recs = [bw.encode_record(W._read("ok%d" % k, 50_000 + k))[0] for k in range(6)]
    members = [bw.bgzf_block(head)] + [bw.bgzf_block(recs[k] + recs[k + 1]) for k in (0, 2, 4)] + [bw.BGZF_EOF]
    return members, np.cumsum([0] + [len(m) for m in members]).tolist()


def _first_data_member(members):
    return 1


def _one_site(path):
    sample, nbam = W.open_sample(path, W.INFO)
    return [{"breakpoint": W.SITE}], sample, nbam


def test_corner_chunk_end_with_in_block_offset_zero(tmp_path):
    members, offs = _corner_bam(tmp_path)
    k = _first_data_member(members)
    assert len(members) - 1 - k >= 2, "the reads must fill several blocks"
    # the chunk ends at the START of the EOF member: in-block offset 0 names the block behind the last one needed
    path = _reindex(tmp_path, "end0", members, [(offs[k] << 16, offs[len(members) - 1] << 16)])
    want, _ = _compare(*_one_site(path), nr.COUNT_SSO, None)
    assert len(want[1]) > 0
    # ... and at the start of a data block in the middle: the reads behind it are not the fetch's
    path = _reindex(tmp_path, "end0mid", members, [(offs[k] << 16, offs[k + 1] << 16)])
    want_mid, _ = _compare(*_one_site(path), nr.COUNT_SSO, None)
    assert 0 < len(want_mid[1]) < len(want[1])


def test_corner_chunk_end_inside_the_eof_member(tmp_path):
    members, offs = _corner_bam(tmp_path)
    k = _first_data_member(members)
    path = _reindex(tmp_path, "ineof", members, [(offs[k] << 16, offs[len(members) - 1] << 16 | 17)])
    want, _ = _compare(*_one_site(path), nr.COUNT_SSO, None)
    assert len(want[1]) > 0


def test_corner_first_offset_beyond_the_blocks_isize(tmp_path):
    members, offs = _corner_bam(tmp_path)
    k = _first_data_member(members)
    isize = I.split_member(members[k])[1]
    # exactly at the block's end: the first record is the next block's first
    path = _reindex(tmp_path, "atend", members, [(offs[k] << 16 | isize, offs[len(members) - 1] << 16)])
    _compare(*_one_site(path), nr.COUNT_SSO, None)
    # beyond it: the unit is the host reader's
    path = _reindex(tmp_path, "beyond", members, [(offs[k] << 16 | (isize + 9), offs[len(members) - 1] << 16)])
    sites, sample, nbam = _one_site(path)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    got = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert nr.WALK_REASONS[int(got[3][0])] == "range" and got[0].tolist() == [0, 0]


def test_corner_record_cut_by_the_end_of_the_data(tmp_path):
    sites, sample, nbam = W.truncated_input(tmp_path)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    closed = nbam.evidence_walk_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    opened = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], None, nr.COUNT_SSO, a[4], 20, 3, 1)
    assert nr.WALK_REASONS[int(opened[3][0])] == "range" and opened[3].tolist() == closed[3].tolist()


def corrupted_fixture(tmp_path):
    """the fixture BAM with one payload byte of a data member in the middle of the file replaced so that it no longer inflates;
    returns (path, offset of that member)"""
    members = _members_of(W.FIXTURE_BAM)
    k = len(members) // 2
    payload, isize = I.split_member(members[k])
    bad = bytearray(members[k])
    at = 18 + len(payload) // 2
    for delta in range(1, 256):
        bad[at] = (members[k][at] + delta) & 0xFF
        if not I.reference(*I.split_member(bytes(bad)))[0]:
            break
    else:
        raise AssertionError("no corrupting byte found")
    path = str(tmp_path / "corrupt.bam")
    with open(path, "wb") as f:
        f.write(b"".join(members[:k] + [bytes(bad)] + members[k + 1:]))
    with open(path + ".bai", "wb") as f:
        f.write(open(W.FIXTURE_BAM + ".bai", "rb").read())
    return path, sum(len(m) for m in members[:k])


def test_a_corrupted_member_flags_the_units_over_it_and_no_others(tmp_path):
    import json
    sites, _sample, _nbam = W.fixture_input()
    path, _at = corrupted_fixture(tmp_path)
    info = json.load(open(os.path.join(W.DATA, "NA12878.bam.json")))
    sample, nbam = W.open_sample(path, info)
    clean_sample, clean = W.open_sample(W.FIXTURE_BAM, info)
    a = W.unit_arrays(sites, sample, nbam, nr.COUNT_SSO)
    want = clean.evidence(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    got = nbam.evidence_walk_open_host(a[0], a[1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 2)
    flagged = got[3] != 0
    assert flagged.any() and not flagged.all()
    assert {nr.WALK_REASONS[int(r)] for r in got[3][flagged]} == {"range"}
    for u in np.flatnonzero(~flagged):
        assert got[1][int(got[0][u]):int(got[0][u + 1])].tobytes() == want[1][int(want[0][u]):int(want[0][u + 1])].tobytes()
        assert got[2][u] == want[2][u]
    # every unit the host reader itself cannot read lies over the member, so it is among the flagged ones
    for u in np.flatnonzero(~flagged)[:40]:
        one = nbam.evidence(a[0][u:u + 1], a[1][u:u + 1], a[2], a[3], 1000, nr.COUNT_SSO, a[4], 20, 3, 1)
        assert one[1].tobytes() == want[1][int(want[0][u]):int(want[0][u + 1])].tobytes()

"""The sync marks of svt_inflate.h, audited on the CPU.  On the device a marked match (bit 15 of b_len) is the only thing between
one lane's loads and another lane's stores inside a batch; on the host a missing mark changes no byte, so no test of bytes can
see it.  tests/native/inflate_marks_main.cpp drives the header's own steps in inflate_member's order and checks the property by
brute force behind every decode_batch; this file builds it with g++ and requires, on every stream of the token corpus (those too
large for a BGZF member included), of zlib_members() and of the fixture BAM: the driver's bytes and statuses are
svt_bgzf_inflate_host's, no violation, marks on the chain cases -- and, with the marks erased (the program's self-check), that
the audit reports the violations."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import inflatecases as I
from svtyper_amd import native_reads as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "svtyper_amd", "csrc")
FIELDS = ("status", "member_status", "same", "batches", "matches", "marked", "violations", "unnecessary")


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("marks")
    exe = str(tmp / "inflate_marks")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "inflate_marks_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "ubsan" in r.stderr.lower()):      # (a g++ without the sanitizer runtimes)
        r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "native", "inflate_marks_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(streams, erase=False):
        """streams: [(label, payload, isize)] -> ({label: figures}, [(status, bytes)])"""
        src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(src, "wb") as f:
            for label, payload, isize in streams:
                name = label.encode()
                f.write(struct.pack("<I", len(name)) + name + struct.pack("<II", len(payload), isize) + payload)
        r = subprocess.run([exe, src, dst] + (["--erase"] if erase else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        figures = {}
        for line in r.stdout.splitlines():
            cells = line.split("\t")
            figures[cells[0]] = dict(zip(FIELDS, map(int, cells[1:])))
        blob, at, outs = open(dst, "rb").read(), 0, []
        for _s in streams:
            status, n = struct.unpack_from("<II", blob, at)
            outs.append((status, blob[at + 8:at + 8 + n]))
            at += 8 + n
        assert at == len(blob) and len(figures) == len(streams)
        return figures, outs
    return run


def _members():
    """[(label, member)]: the token corpus good and bad, the handmade bad streams, what zlib writes, the fixture BAM"""
    return ([(label, m) for label, m, _raw in I.token_members() + I.zlib_members() + I.bam_members([I.W.FIXTURE_BAM])] +
            I.token_bad_members() + I.handmade_bad_members())


def _streams(members):
    return [(label,) + I.split_member(m) for label, m in members]


def test_the_driver_is_inflate_member(audit):
    """bytes and statuses of the audited drive are svt_bgzf_inflate_host's, on good and bad streams"""
    members = _members()
    figures, outs = audit(_streams(members))
    data, block_off, out_off = I.layout([m for _label, m in members])
    out, status = nr.bgzf_inflate(data, block_off, out_off)
    for k, (label, _m) in enumerate(members):
        assert figures[label]["same"] == 1 and figures[label]["status"] == figures[label]["member_status"], (label, figures[label])
        assert outs[k][0] == status[k], "%s: status %d, svt_bgzf_inflate_host %d" % (label, outs[k][0], status[k])
        if status[k] == 0:
            assert outs[k][1] == out[int(out_off[k]):int(out_off[k + 1])].tobytes(), label + ": bytes differ"
    assert int(np.count_nonzero(status)) >= 23 and int(np.count_nonzero(status == 0)) >= 60 + 46 + 70


def test_streams_too_large_for_a_member_inflate_byte_for_byte(audit):
    """a stored block of LEN 65 535, and ISIZE 65 536 from it and one literal: zlib's bytes, from the drive and from
    inflate_member<HostCtx> (the program compares the two)"""
    cases = I.oversize_payloads()
    figures, outs = audit([(label, payload, len(raw)) for label, payload, raw in cases])
    for k, (label, payload, raw) in enumerate(cases):
        assert len(payload) > I.MAX_PAYLOAD
        assert outs[k] == (0, raw) and figures[label]["same"] == 1 and figures[label]["member_status"] == 0, label
    assert {len(raw) for _l, _p, raw in cases} == {65535, 65536}
    # ... and one byte short / one byte over of room is refused
    label, payload, raw = cases[1]
    _figures, outs = audit([("short", payload, len(raw) - 1), ("cut", payload[:-1], len(raw))])
    assert [s for s, _b in outs] == [7, 1]


def test_no_match_reads_what_an_unsynced_match_wrote(audit):
    members = [(label, m) for label, m in _members() if I.reference(*I.split_member(m))[0]]
    streams = _streams(members) + [(label, payload, len(raw)) for label, payload, raw in I.oversize_payloads()]
    figures, _outs = audit(streams)
    total = {f: sum(v[f] for v in figures.values()) for f in FIELDS[3:]}
    print("streams", len(streams), total)
    bad = {label: v for label, v in figures.items() if v["violations"] or v["status"]}
    assert not bad, bad
    chains = [label for label in figures if label.startswith("chain/")]
    assert len(chains) == 24
    for label in chains:
        assert figures[label]["marked"] > 0, label
    # (one batch: a literal and 127 matches, each but the first reading the one before)
    assert figures["chain/127/fixed/j0"]["marked"] == 126 and figures["chain/127/dynamic/j0"]["marked"] == 126
    assert total["marked"] > 30000                             # (what zlib writes reaches tens of thousands of marked matches)


def test_the_audit_sees_a_missing_mark(audit):
    """the self-check: with every batch's marks erased the audit reports violations on every chain case, and the bytes -- one
    lane, no race to lose -- stay right, which is why only the audit can see it"""
    members = [(label, m) for label, m, _raw in I.token_members() if label.startswith("chain/")]
    figures, outs = audit(_streams(members), erase=True)
    raws = {label: raw for label, _m, raw in I.token_members()}
    for k, (label, _m) in enumerate(members):
        assert figures[label]["violations"] > 0 and figures[label]["marked"] == 0, (label, figures[label])
        assert outs[k] == (0, raws[label]), label
    assert figures["chain/127/fixed/j0"]["violations"] == 126

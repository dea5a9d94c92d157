"""The dynamic-Huffman mode of the BGZF compressor on the host: svt_bgzf_deflate_host_mode(SVT_DEFLATE_DYNAMIC)
(svtyper_amd/csrc/svt_deflate.h on the CPU) against the Python restatement of DESIGN 3.4 (tests/dynhuffcases.py), byte for byte
over the whole corpus; its output inflated by zlib and by the plain reference inflater; mode 0 against the old entry; the
code-length rule on its own (svt_huffman_lengths_host) against the restatement, Kraft sums and the Huffman optimum; the refusals;
and the Python writers with huffman="dynamic".  No GPU."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import deflatecases as D  # noqa: E402
import deflatewriter as dw  # noqa: E402
import dynhuffcases as H  # noqa: E402
from svtyper_amd import bam, bgzf_out, hip  # noqa: E402
from svtyper_amd import native_reads as nr  # noqa: E402

DATA = os.path.join(HERE, "data")


@pytest.fixture(scope="module")
def cases():
    return H.corpus()


@pytest.fixture(scope="module")
def host(cases):
    """(members, out_off) of the corpus in one call, dynamic mode"""
    return nr.bgzf_deflate([p for _name, p in cases], huffman="dynamic")


def split(members, out_off):
    return [members[int(out_off[k]):int(out_off[k + 1])].tobytes() for k in range(len(out_off) - 1)]


def test_the_corpus_reaches_what_the_format_names(cases):
    got, least = H.reach(cases)
    assert not H.REACH["flags"] - got, sorted(H.REACH["flags"] - got)
    assert 12 <= least <= H.HCLEN_LEAST


def test_host_bytes_are_the_restatements(cases, host):
    got = split(*host)
    assert len(got) == len(cases)
    for (name, p), member in zip(cases, got):
        assert member == H.member(p), name


def test_zlib_and_the_reference_inflater_return_the_payloads(cases, host):
    blocks = set()
    for (name, p), member in zip(cases, split(*host)):
        cdata = member[18:-8]
        assert zlib.decompress(cdata, -15) == p, name
        assert gzip.decompress(member) == p, name
        blocks.add(cdata[0] >> 1 & 3)
        if len(p) <= 4096 or cdata[0] >> 1 & 3 == 2 and len(p) <= 20000:       # (bit by bit in Python: the short ones, all kinds)
            ok, out, _profile = dw.inflate(cdata, len(p))
            assert ok and out == p, name
    assert blocks == {0, 1, 2}


def test_mode_0_is_the_old_entry(cases):
    payloads = [p for _name, p in cases]
    old, old_off = nr.bgzf_deflate(payloads)
    L = nr._lib()
    data = np.frombuffer(b"".join(payloads), np.uint8)
    off = np.cumsum([0] + [len(p) for p in payloads]).astype(np.uint64)
    out = np.zeros(data.size + 31 * len(payloads), np.uint8)
    out_off = np.zeros(len(payloads) + 1, np.uint64)
    assert L.svt_bgzf_deflate_host_mode(data.ctypes.data, off.ctypes.data, len(payloads), out.ctypes.data, out.size, out_off.ctypes.data, 0) == 0
    assert np.array_equal(out_off, old_off) and np.array_equal(out[:int(out_off[-1])], old)


def test_no_dynamic_member_is_longer_than_the_fixed_modes(cases, host):
    _old, old_off = nr.bgzf_deflate([p for _name, p in cases])
    shorter = 0
    for k, (name, _p) in enumerate(cases):
        assert host[1][k + 1] - host[1][k] <= old_off[k + 1] - old_off[k], name
        shorter += host[1][k + 1] - host[1][k] < old_off[k + 1] - old_off[k]
    assert shorter > 0


def test_every_member_of_the_vcf_text_is_strictly_shorter():
    with open(os.path.join(DATA, "example.gt.vcf"), "rb") as f:
        text = f.read()
    text = text * (3 * D.MAX_PAYLOAD // len(text) + 1)
    payloads = [text[k * D.MAX_PAYLOAD:(k + 1) * D.MAX_PAYLOAD] for k in range(3)]
    fixed, dynamic = nr.bgzf_deflate(payloads)[1], nr.bgzf_deflate(payloads, huffman="dynamic")[1]
    sizes = [(int(fixed[k + 1] - fixed[k]), int(dynamic[k + 1] - dynamic[k])) for k in range(3)]
    print("members of 65 280 bytes of VCF text, (fixed, dynamic) bytes:", sizes)
    assert all(d < f for f, d in sizes)
    assert sum(d for _f, d in sizes) <= 0.33 * 3 * D.MAX_PAYLOAD       # (the fixed block is 0.43 of it, the CPU estimate 0.30)


def test_no_payload_stays_the_eof_member():
    members, out_off = nr.bgzf_deflate([b""], huffman="dynamic")
    assert members.tobytes() == bam.BGZF_EOF and list(out_off) == [0, 28]
    assert list(nr.bgzf_deflate([], huffman="dynamic")[1]) == [0]


def test_huffman_lengths_are_the_restatements_and_sound():
    deep = 0
    for limit in (7, 15):
        sets = [(name, f) for name, f, lim in H.histograms() if lim == limit]
        for symbols in sorted({len(f) for _name, f in sets}):
            group = [(name, f) for name, f in sets if len(f) == symbols]
            got = nr.huffman_lengths(np.array([f for _name, f in group], np.uint32), limit)
            assert got.shape == (len(group), symbols)
            for (name, f), lens in zip(group, got.tolist()):
                assert lens == H.lengths(list(f), limit), name
                assert H.kraft_ok(lens, limit), name
                assert all((l > 0) == (x > 0) for l, x in zip(lens, f)), name
                best, depth = H.optimum(f)
                if depth <= limit:
                    assert H.cost(f, lens) == best, name
                else:
                    deep += 1
                    assert H.cost(f, lens) > best, name
    assert deep >= 6                            # (the Fibonacci ones over 286, 30 and 19 symbols, and one level too deep)
    one = nr.huffman_lengths(np.array([0, 3, 0], np.uint32), 15)
    assert one.shape == (3,) and one.tolist() == [0, 1, 0]


def test_the_deep_histograms_are_deep():
    names = {name: (f, limit) for name, f, limit in H.histograms()}
    for name in ("fibonacci-286", "fibonacci-286-dense", "fibonacci-30", "fibonacci-30-reversed", "fibonacci-19", "depth-16", "depth-8"):
        f, limit = names[name]
        assert H.optimum(f)[1] > limit, name
    for name in ("depth-15", "depth-7"):
        f, limit = names[name]
        assert H.optimum(f)[1] == limit, name


@pytest.mark.parametrize("what", ["mode", "limit", "symbols", "sum", "used"])
def test_refusals_of_the_c_abi(what):
    L = nr._lib()
    if what == "mode":
        data, off = np.zeros(8, np.uint8), np.array([0, 8], np.uint64)
        out, out_off = np.full(64, 0xEE, np.uint8), np.zeros(2, np.uint64)
        rc = L.svt_bgzf_deflate_host_mode(data.ctypes.data, off.ctypes.data, 1, out.ctypes.data, out.size, out_off.ctypes.data, 2)
        assert rc != 0 and (out == 0xEE).all()
        with pytest.raises(hip.SvtyperHipError, match="mode"):
            hip._check(rc)
        return
    call = {"limit": lambda: nr.huffman_lengths([1, 2, 3], 9),
            "symbols": lambda: nr.huffman_lengths([1] * 287, 15),
            "sum": lambda: nr.huffman_lengths([0xFFFFFFFF, 1], 15),
            "used": lambda: nr.huffman_lengths([1] * 129, 7)}[what]
    with pytest.raises(hip.SvtyperHipError):
        call()


def test_dynamic_with_zlib_and_an_unknown_huffman_are_refused(tmp_path):
    for make in (lambda **kw: bam.BgzfWriter(str(tmp_path / "a.gz"), **kw), lambda **kw: bgzf_out.open_text(str(tmp_path / "b.gz"), **kw)):
        with pytest.raises(ValueError, match="huffman"):
            make(huffman="dynamic")
        with pytest.raises(ValueError, match="huffman"):
            make(deflate="zlib", huffman="dynamic")
        with pytest.raises(ValueError, match="huffman"):
            make(deflate="host", huffman="bogus")
    with pytest.raises(ValueError, match="huffman"):
        nr.bgzf_deflate([b"abc"], huffman="bogus")
    import test_host_pipeline as T
    import test_write_alignment_host as W
    with pytest.raises(ValueError, match="huffman"):
        W.run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, str(tmp_path / "w.bam"), huffman="dynamic")
    assert not os.path.exists(str(tmp_path / "a.gz")) and not os.path.exists(str(tmp_path / "w.bam"))


def test_the_writers_with_the_dynamic_block(tmp_path):
    with open(os.path.join(DATA, "example.gt.vcf"), "rb") as f:
        text = f.read()
    sizes = {}
    for huffman in ("fixed", "dynamic"):
        path = str(tmp_path / (huffman + ".gz"))
        w = bam.BgzfWriter(path, deflate="host", huffman=huffman)
        w.write(text * 3)
        w.close()
        raw = open(path, "rb").read()
        assert gzip.decompress(raw) == text * 3 and raw.endswith(bam.BGZF_EOF)
        sizes[huffman] = len(raw)
        path = str(tmp_path / (huffman + ".vcf.gz"))
        out = bgzf_out.open_text(path, deflate="host", huffman=huffman)
        out.write(text.decode() * 2)
        out.close()
        raw = open(path, "rb").read()
        assert gzip.decompress(raw) == text * 2 and raw.endswith(bam.BGZF_EOF)
    assert sizes["dynamic"] < sizes["fixed"]


def test_the_command_line_knows_the_option(monkeypatch):
    from svtyper_amd import classic, singlesample
    for program in (classic, singlesample):
        monkeypatch.setattr(sys, "argv", ["svtyper", "-i", os.path.join(DATA, "example.vcf"), "-B", "x.bam"])
        assert program.get_args().huffman == "fixed"
        monkeypatch.setattr(sys, "argv", sys.argv + ["--deflate", "host", "--huffman", "dynamic"])
        assert program.get_args().huffman == "dynamic"
        monkeypatch.setattr(sys, "argv", sys.argv[:-1] + ["bogus"])
        with pytest.raises(SystemExit):
            program.get_args()

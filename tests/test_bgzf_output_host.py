"""BGZF output on the host: the VCF of sv_genotype / sso_genotype through bgzf_out.open_text, and the `-w` BAM through
bam.BgzfWriter, with deflate="host" (the library's own compressor, svt_deflate.h, on the CPU) and deflate="zlib".  No GPU: the
engine seam is filled by the oracle engines the other host tests use."""
import gzip
import io
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import test_host_pipeline as T  # noqa: E402
import test_write_alignment_host as W  # noqa: E402
from svtyper_amd import bam, bgzf_out, classic, singlesample  # noqa: E402


def no_date(text):
    return [l for l in text.split("\n") if not l.startswith("##fileDate=")]


def run(driver, out):
    with open(T.IN_VCF) as inf:
        if driver == "classic":
            classic.sv_genotype(T.IN_BAM, inf, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, None, False, None, 1e10,
                                engine=T.oracle_engine, reader="python")
        else:
            singlesample.sso_genotype(T.IN_BAM, inf, out, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000,
                                      engine=T.oracle_engine, reader="python")


@pytest.fixture(scope="module")
def plain():
    out = {}
    for driver in ("classic", "sso"):
        sink = io.StringIO()
        sink.close = lambda: None
        run(driver, sink)
        out[driver] = sink.getvalue()
    return out


@pytest.mark.parametrize("deflate", ["host", "zlib"])
@pytest.mark.parametrize("driver", ["classic", "sso"])
def test_vcf_through_open_text(tmp_path, plain, driver, deflate):
    path = str(tmp_path / "out.vcf.gz")
    out = bgzf_out.open_text(path, deflate=deflate)
    run(driver, out)
    out.close()
    with open(path, "rb") as f:
        raw = f.read()
    assert no_date(gzip.decompress(raw).decode()) == no_date(plain[driver])
    assert raw.endswith(bam.BGZF_EOF)
    sizes = W.members(path)
    assert sizes[-1][2] == 0 and all(size <= 0x10000 for _at, size, _isize in sizes)
    assert all(isize == 0xff00 for _at, _size, isize in sizes[:-2])        # cut every 65 280 bytes, whoever compresses


def test_open_text_over_a_file_object_and_flush(tmp_path):
    path = str(tmp_path / "t.gz")
    with open(path, "wb") as f:
        out = bgzf_out.open_text(f, deflate="host")
        out.write("one\n")
        out.flush()
        assert gzip.decompress(open(path, "rb").read()) == b"one\n"
        out.write("two\n" * 40000)
        out.close()
        out.close()
        assert f.closed
    assert gzip.decompress(open(path, "rb").read()) == b"one\n" + b"two\n" * 40000
    assert [isize for _at, _size, isize in W.members(path)] == [4, 0xff00, 0xff00, 160000 - 2 * 0xff00, 0]


@pytest.fixture(scope="module")
def w_files(tmp_path_factory):
    """the fixture's `-w` BAM (reader="python") with no deflate given, with "zlib" and with "host": {name: bytes}, and the paths"""
    tmp = tmp_path_factory.mktemp("w")
    paths = {name: str(tmp / (name + ".bam")) for name in ("default", "zlib", "host")}
    for name, path in paths.items():
        W.run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, path, **({} if name == "default" else {"deflate": name}))
    return {name: open(path, "rb").read() for name, path in paths.items()}, paths


def test_write_alignment_host_is_zlibs_payload_in_the_same_members(w_files):
    raw, paths = w_files
    assert gzip.decompress(raw["host"]) == gzip.decompress(raw["zlib"])
    assert [m[2] for m in W.members(paths["host"])] == [m[2] for m in W.members(paths["zlib"])]
    assert raw["host"] != raw["zlib"] and raw["host"].endswith(bam.BGZF_EOF)


def test_the_default_writes_what_zlib_writes(w_files):
    raw, _paths = w_files
    assert raw["default"] == raw["zlib"]


def test_run_main_wraps_the_output_only_when_asked(tmp_path):
    import argparse
    from svtyper_amd import driver
    seen = []

    def fake(bam_string, vcf_in, vcf_out, **options):
        seen.append(type(vcf_out).__name__)
        vcf_out.write("line\n" * 3)

    for bgzf in (False, True):
        path = str(tmp_path / ("out%d" % bgzf))
        args = argparse.Namespace(split_bam=None, geometry="host", reader=None, inflate="host", library_scan="host", verify_bgzf=False,
                                  bgzf=bgzf, deflate="host")
        out = open(path, "w")
        driver.run_main(fake, None, ("b", None, out), args)
        out.close()
        data = open(path, "rb").read()
        assert (gzip.decompress(data) if bgzf else data) == b"line\n" * 3
        assert not bgzf or data.endswith(bam.BGZF_EOF)
    assert seen == ["TextIOWrapper", "BgzfTextWriter"]


def test_nothing_of_it_is_imported_without_the_options():
    import subprocess
    code = ("import sys, svtyper_amd.classic, svtyper_amd.singlesample, svtyper_amd.bam; "
            "assert 'svtyper_amd.bgzf_out' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_an_unknown_deflate_is_refused(tmp_path):
    with pytest.raises(ValueError, match="deflate"):
        W.run_w(T.IN_BAM, T.IN_VCF, T.LIB_JSON, str(tmp_path / "w.bam"), deflate="bogus")
    with pytest.raises(ValueError, match="deflate"):
        bgzf_out.open_text(str(tmp_path / "x.gz"), deflate="bogus")
    with pytest.raises(ValueError, match="deflate"):
        bam.BgzfWriter(str(tmp_path / "y.gz"), deflate="bogus")

"""inflate="device" is only legal with reader="device": every driver says so before it opens anything (no GPU needed)."""
import io

import pytest

import test_host_pipeline as H
from svtyper_amd import pipeline


@pytest.mark.parametrize("reader", ["python", "native", None])
def test_inflate_device_needs_the_device_reader(tmp_path, reader):
    for run in (lambda **kw: H.run_classic(str(tmp_path / "c.vcf"), H.oracle_engine, **kw),
                lambda **kw: H.run_sso(str(tmp_path / "s.vcf"), H.oracle_engine, None, **kw)):
        with pytest.raises(ValueError, match="only legal with reader='device'"):
            run(reader=reader, inflate="device")
    with pytest.raises(ValueError, match="inflate must be"):
        H.run_classic(str(tmp_path / "c.vcf"), H.oracle_engine, reader="device", inflate="gpu")


def test_the_default_is_the_host():
    assert pipeline.check_inflate("native", "host") == "host" and pipeline.check_inflate("device", "device") == "device"
    with pytest.raises(ValueError):
        pipeline.NativeUnitCollector([], [], 1.0, 1.0, 20, 0, None, geometry="reader", inflate="device")

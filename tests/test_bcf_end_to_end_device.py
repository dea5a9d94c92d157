"""GPU: sso_genotype and sv_genotype over the fixture with open_bcf(deflate="device", sort=True, index="csi") as their vcf_out.  The
same run's text is kept beside it: decoded by the independent reader of tests/bcfreader.py, the BCF's records are that text's
data lines in sorted order, field for field (floats bitwise as numpy.float32(float(token))), the header text inside the BCF is
the text route's header, no line left the device, and the .csi leads to every record."""
import io

import pytest

import bcfreader as R
import test_bcf_host as H
import test_host_pipeline as T
from svtyper_amd import bcf_out, classic, singlesample

pytestmark = pytest.mark.gpu


class Both:
    """what the driver writes goes to the BCF writer and is kept as text"""

    def __init__(self, out):
        self.out, self.text = out, io.StringIO()
        self.name = out.name

    def write(self, s):
        self.text.write(s)
        return self.out.write(s)

    def flush(self):
        self.out.flush()

    def close(self):
        self.out.close()


@pytest.mark.parametrize("driver", ["sso", "sv"])
def test_fixture_as_sorted_indexed_bcf(tmp_path, hip_device, driver):
    path = str(tmp_path / (driver + ".bcf"))
    out = bcf_out.open_bcf(path, deflate="device", device=hip_device, sort=True, index="csi")
    both = Both(out)
    with open(T.IN_VCF) as inf:
        if driver == "sso":
            singlesample.sso_genotype(T.IN_BAM, inf, both, 20, 1, 1, 1000000, T.LIB_JSON, False, None, False, 1000, 1e10, None, 1000)
        else:
            classic.sv_genotype(T.IN_BAM, inf, both, 20, 1, 1, 1000000, T.LIB_JSON, False, None, None, False, None, 1e10)
    out.close()
    text = both.text.getvalue()
    assert out.host_lines == 0 and text.count("\n") > 300
    with open(path, "rb") as f:
        head, d, records, _ = R.read_bcf(R.stream_of(f.read()))
    assert head == "".join(l + "\n" for l in text.split("\n") if l.startswith("#")) and len(records) == 212
    contigs = [l for l in text.split("\n") if l.startswith("##contig=<")]
    lengths = [int(R.header_field(l, "length")) for l in contigs]
    assert H.check_indexed(path, text, len(contigs), max(lengths)) > 50

"""What the compiler made of mi_inflate_index.hip, checked without a GPU in the manner of test_kernel_resources_inflate.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The span decoder lives in a file and a kernel of its
own; mi_inflate.hip's kernels and their figures stay test_kernel_resources_inflate.py's."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNEL = "mi::inflate_span_kernel"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_inflate_index.hip", [], str(tmp_path_factory.mktemp("kres_inflate_index")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.22"):]
    return dict((m.group(1), tuple(int(m.group(k).replace(" ", "")) for k in (2, 3, 4, 5))) for m in
                re.finditer(r"^\| `mi::(inflate_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_span_kernel_without_scratch_vgpr_spills_or_agprs(usage):
    assert sorted(usage) == [KERNEL], sorted(usage)
    u = usage[KERNEL]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["AGPRs"] == 0, u
    assert "mi_inflate_index.hip" in open(os.path.join(ROOT, "makisu_amd", "build.py")).read()
    assert "inflate_span_kernel" not in open(os.path.join(CSRC, "mi_inflate.hip")).read()     # the old file's kernel list is what it was


def test_the_span_kernels_lds_is_the_wave_headers(usage):
    head = open(os.path.join(CSRC, "mi_inflate_wave.h")).read()
    lds = int(re.search(r"kInfLds = ([\d ]+) bytes", head).group(1).replace(" ", ""))
    assert usage[KERNEL]["LDS Size [bytes/block]"] == lds == 4384, usage[KERNEL]


def test_the_kernel_keeps_the_figures_the_design_states(usage):
    """DESIGN 4.22's table, as compiled: VGPRs and LDS equal, no more SGPRs spilled (into VGPR lanes: there is no scratch) than stated, at
    least the occupancy stated"""
    rows = _design_rows()
    assert sorted(rows) == ["inflate_span_kernel"]
    vgprs, lds, sgpr_spill, waves = rows["inflate_span_kernel"]
    u = usage[KERNEL]
    assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), u
    assert u["SGPRs Spill"] <= sgpr_spill and u["Occupancy [waves/SIMD]"] >= waves >= 6, u

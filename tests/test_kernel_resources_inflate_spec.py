"""What the compiler made of mi_inflate_spec.hip, checked without a GPU in the manner of test_kernel_resources_inflate_index.py:
registers, spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The speculative inflate lives in a file
and in kernels of its own; the other inflate files' kernels and figures stay their own tests'."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNELS = ["mi::inflate_find_kernel", "mi::inflate_spec_windows_kernel", "mi::inflate_speculate_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_inflate_spec.hip", [], str(tmp_path_factory.mktemp("kres_inflate_spec")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.23"):]
    return dict((m.group(1), tuple(int(m.group(k).replace(" ", "")) for k in (2, 3, 4, 5))) for m in
                re.finditer(r"^\| spec: `(inflate_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_three_kernels_without_scratch_vgpr_spills_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)
    assert "mi_inflate_spec.hip" in open(os.path.join(ROOT, "makisu_amd", "build.py")).read()
    for other in ("mi_inflate.hip", "mi_inflate_index.hip"):
        text = open(os.path.join(CSRC, other)).read()
        assert "__global__" in text and not any(k[4:] in text for k in KERNELS), other       # the older files' kernel lists are what they were


def test_the_lds_is_the_wave_headers_plus_the_staging_of_entries(usage):
    head = open(os.path.join(CSRC, "mi_inflate_wave.h")).read()
    lds = int(re.search(r"kInfLds = ([\d ]+) bytes", head).group(1).replace(" ", ""))
    assert usage["mi::inflate_find_kernel"]["LDS Size [bytes/block]"] == lds
    assert usage["mi::inflate_speculate_kernel"]["LDS Size [bytes/block]"] == lds + 2 * 512    # kInfRing u16 entries
    assert usage["mi::inflate_spec_windows_kernel"]["LDS Size [bytes/block]"] == 0
    assert 7 * 4 * (lds + 1024) <= 160 * 1024 < 8 * 4 * (lds + 1024)                           # seven waves a SIMD fit a CU's 160 KiB, not eight


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.23's table, as compiled: VGPRs and LDS equal, no more SGPRs spilled (into VGPR lanes: there is no scratch) than stated, at
    least the occupancy stated"""
    rows = _design_rows()
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds, sgpr_spill, waves) in rows.items():
        u = usage["mi::" + k]
        assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), (k, u)
        assert u["SGPRs Spill"] <= sgpr_spill and u["Occupancy [waves/SIMD]"] >= waves >= 6, (k, u)

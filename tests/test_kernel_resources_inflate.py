"""What the compiler made of mi_inflate.hip, checked without a GPU in the manner of test_kernel_resources_deflate.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The existing files' resource tests are
untouched: the device inflate lives in kernels of its own, named inflate_*."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNELS = ["mi::inflate_mark_count_kernel", "mi::inflate_mark_scan_kernel", "mi::inflate_mark_scatter_kernel", "mi::inflate_size_kernel",
           "mi::inflate_table_kernel", "mi::inflate_write_kernel"]
WAVE = ("mi::inflate_size_kernel", "mi::inflate_write_kernel", "mi::inflate_table_kernel")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_inflate.hip", [], str(tmp_path_factory.mktemp("kres_inflate")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.20"):]
    return dict((m.group(1), tuple(int(m.group(k).replace(" ", "")) for k in (2, 3, 4, 5))) for m in
                re.finditer(r"^\| `(inflate_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_inflate_kernels_without_scratch_vgpr_spills_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)
        if name not in WAVE[:2]:
            assert u["SGPRs Spill"] == 0, (name, u)
    assert "mi_inflate.hip" in open(os.path.join(ROOT, "makisu_amd", "build.py")).read()
    deflate = open(os.path.join(CSRC, "mi_deflate.hip")).read()
    assert "inflate" not in deflate                                                          # the two legs share no file


def test_the_wave_kernels_lds_is_what_the_header_states_and_within_the_target(usage):
    head = open(os.path.join(CSRC, "mi_inflate_wave.h")).read()
    lds = int(re.search(r"kInfLds = ([\d ]+) bytes", head).group(1).replace(" ", ""))
    for name in WAVE:
        assert usage[name]["LDS Size [bytes/block]"] == lds == 4384, (name, usage[name])
    assert lds <= 5120 and 8 * 4 * lds <= 160 * 1024                                         # eight waves a SIMD fit a CU's 160 KiB
    for name in KERNELS[:3]:
        assert usage[name]["LDS Size [bytes/block]"] <= 64, (name, usage[name])              # the block sums' and the scan's few words


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.20's table, as compiled: VGPRs and LDS equal, no more SGPRs spilled (into VGPR lanes: there is no scratch) than stated,
    and every kernel reaches at least the occupancy stated for it"""
    rows = _design_rows()
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds, sgpr_spill, waves) in rows.items():
        u = usage["mi::" + k]
        assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), (k, u)
        assert u["SGPRs Spill"] <= sgpr_spill and u["Occupancy [waves/SIMD]"] >= waves, (k, u)
    assert rows["inflate_size_kernel"][3] >= 6 and rows["inflate_write_kernel"][3] >= 6

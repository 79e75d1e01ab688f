"""What the compiler made of mi_deflate.hip, checked without a GPU in the manner of test_kernel_resources_zserve.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The existing files' resource tests are
untouched: the device deflate leg lives in kernels of its own."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNELS = ["mi::deflate_code_lengths_kernel", "mi::deflate_emit_kernel", "mi::deflate_offsets_kernel", "mi::deflate_plan_kernel",
           "mi::deflate_scan_kernel", "mi::deflate_sums_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_deflate.hip", [], str(tmp_path_factory.mktemp("kres_deflate")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.19"):]
    return dict((m.group(1), (int(m.group(2)), int(m.group(3).replace(" ", "")), int(m.group(4)))) for m in
                re.finditer(r"^\| `(deflate_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_deflate_kernels_without_spills_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)
    assert "mi_deflate.hip" in open(os.path.join(ROOT, "makisu_amd", "build.py")).read()


def test_the_wave_kernels_lds_is_what_the_header_states(usage):
    head = open(os.path.join(CSRC, "mi_deflate_wave.h")).read()
    plan = int(re.search(r"kDfPlanLds = ([\d ]+) bytes", head).group(1).replace(" ", ""))
    emit = int(re.search(r"kDfEmitLds = ([\d ]+) bytes", head).group(1).replace(" ", ""))
    assert usage["mi::deflate_plan_kernel"]["LDS Size [bytes/block]"] == plan == 23088       # table + counts + codes + header
    assert usage["mi::deflate_code_lengths_kernel"]["LDS Size [bytes/block]"] == plan        # (the probe's kernel borrows the plan's)
    assert usage["mi::deflate_emit_kernel"]["LDS Size [bytes/block]"] == emit == 1440        # codes + lengths + staging
    for name in ("mi::deflate_sums_kernel", "mi::deflate_scan_kernel", "mi::deflate_offsets_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] <= 64, (name, usage[name])              # the block sums' and the scan's few words


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.19's table, as compiled: VGPRs and LDS equal, and every kernel reaches at least the occupancy stated for it"""
    rows = _design_rows()
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds, waves) in rows.items():
        u = usage["mi::" + k]
        assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), (k, u)
        assert u["Occupancy [waves/SIMD]"] >= waves, (k, u)
    assert rows["deflate_emit_kernel"][2] == 8 and rows["deflate_plan_kernel"][2] >= 1

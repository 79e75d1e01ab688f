"""What the compiler made of mi_tarscan.hip, checked without a GPU in the manner of test_kernel_resources_inflate.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  mi_layerblob.hip holds no kernel of its own; the
device destination of the inflater added none to mi_inflate.hip (test_kernel_resources_inflate.py lists that file's)."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["mi::tar_count_kernel", "mi::tar_gather_kernel", "mi::tar_mark_kernel", "mi::tar_scan_kernel", "mi::tar_scatter_kernel"]
SCAN = ("mi::tar_count_kernel", "mi::tar_scan_kernel", "mi::tar_scatter_kernel")


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_tarscan.hip", [], str(tmp_path_factory.mktemp("kres_tarscan")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.21"):]
    return dict((m.group(1), tuple(int(m.group(k).replace(" ", "")) for k in (2, 3, 4))) for m in
                re.finditer(r"^\| `(tar_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_tar_kernels_without_scratch_or_spills(usage, tmp_path):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)
    build = open(os.path.join(ROOT, "makisu_amd", "build.py")).read()
    assert "mi_tarscan.hip" in build and "mi_layerblob.hip" in build
    assert _usage("mi_layerblob.hip", [], str(tmp_path)) == {}


def test_lds_is_the_scans_and_nothing_else(usage):
    for name in KERNELS:
        lds = usage[name]["LDS Size [bytes/block]"]
        assert lds == (32 if name in SCAN else 0), (name, usage[name])      # the block sums' or the block scan's four words


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.21's table, as compiled: VGPRs and LDS equal, and every kernel reaches at least the occupancy stated for it"""
    rows = _design_rows()
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds, waves) in rows.items():
        u = usage["mi::" + k]
        assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), (k, u)
        assert u["Occupancy [waves/SIMD]"] >= waves, (k, u)
    assert rows["tar_mark_kernel"][2] >= 8                                 # memory-bound: every wave slot of a SIMD is used

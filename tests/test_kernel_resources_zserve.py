"""What the compiler made of mi_zserve.hip, checked without a GPU in the manner of test_kernel_resources_zentropy.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The existing files' resource tests are
untouched: the two cuts live in kernels of their own."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNELS = ["mi::zcut_compare_kernel", "mi::zcut_decode_kernel", "mi::zcut_entries_kernel", "mi::zcut_gather_kernel", "mi::zcut_offsets_kernel",
           "mi::zcut_sizes_kernel", "mi::zcut_unwrap_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zserve.hip", [], str(tmp_path_factory.mktemp("kres_zserve")))


def _design_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.17"):]
    return dict((m.group(1), (int(m.group(2)), int(m.group(3).replace(" ", "")), int(m.group(4)))) for m in
                re.finditer(r"^\| `(zcut_\w+)` \| (\d+) \| ([\d ]+) \| (\d+) \|", section, re.M))


def test_the_file_compiles_exactly_the_zcut_kernels_without_spills_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)
    assert "zcut_" in open(os.path.join(CSRC, "mi_zserve.hip")).read() and "mi_zserve.hip" in open(os.path.join(ROOT, "makisu_amd", "build.py")).read()


def test_the_wave_kernels_lds_is_the_unwrap_table_and_the_gathers_is_the_tiles(usage):
    head = open(os.path.join(CSRC, "mi_huff_wave.h")).read()
    m = re.search(r"kZhUnwrapLds = ([\d ]+) bytes", head)
    total = int(m.group(1).replace(" ", ""))
    assert usage["mi::zcut_decode_kernel"]["LDS Size [bytes/block]"] == total == 4928
    assert usage["mi::zcut_unwrap_kernel"]["LDS Size [bytes/block]"] == total
    assert usage["mi::zcut_gather_kernel"]["LDS Size [bytes/block]"] == 16400                # mi_gather.h's tile body
    assert usage["mi::zcut_compare_kernel"]["LDS Size [bytes/block]"] == 0
    for name in ("mi::zcut_sizes_kernel", "mi::zcut_offsets_kernel", "mi::zcut_entries_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] <= 320, (name, usage[name])             # the block sums' and the scan's few words
    assert "kZhUnwrapLds = 4 928 bytes" in open(os.path.join(CSRC, "mi_zserve.hip")).read()


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.17's table, as compiled: VGPRs and LDS equal, and every kernel reaches at least the occupancy stated for it"""
    rows = _design_rows()
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds, waves) in rows.items():
        u = usage["mi::" + k]
        assert (u["VGPRs"], u["LDS Size [bytes/block]"]) == (vgprs, lds), (k, u)
        assert u["Occupancy [waves/SIMD]"] >= waves, (k, u)
    assert rows["zcut_unwrap_kernel"][2] == 8 and rows["zcut_decode_kernel"][2] >= 7 and rows["zcut_gather_kernel"][2] == 8

"""What the compiler made of mi_zentropy.hip, checked without a GPU in the manner of test_kernel_resources_zrecode.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The LZ4 kernels' own resource tests are
untouched: the stage lives in kernels of its own."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")
KERNELS = ["mi::zh_classify_kernel", "mi::zh_encode_kernel", "mi::zh_offsets_kernel", "mi::zh_place_kernel", "mi::zh_recode_encode_kernel",
           "mi::zh_recode_place_kernel", "mi::zh_redecode_kernel", "mi::zh_rep_rows_kernel", "mi::zh_rules_merge_kernel", "mi::zh_sources_kernel", "mi::zh_unwrap_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zentropy.hip", [], str(tmp_path_factory.mktemp("kres_zentropy")))


def test_no_zentropy_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_unwrap_kernels_lds_is_the_table_plus_what_the_file_header_states(usage):
    """4 KiB for the 2 048-entry table and the 832 bytes mi_huff_wave.h's LDS paragraph lists beside it"""
    head = open(os.path.join(CSRC, "mi_huff_wave.h")).read()
    m = re.search(r"kZhUnwrapLds = ([\d ]+) bytes -- the table \(2 048 16-bit entries, 4 KiB\) and (\d+) bytes beside it: 256 code\s*//\s*lengths "
                  r"\((\d+) bytes\), 256 16-bit codes \((\d+) bytes\), 16 counts per length \((\d+) bytes\)", head)
    assert m, "the LDS paragraph of mi_huff_wave.h"
    total, beside, parts = int(m.group(1).replace(" ", "")), int(m.group(2)), [int(m.group(i)) for i in (3, 4, 5)]
    assert sum(parts) == beside == 832 and total == 2048 * 2 + beside
    assert usage["mi::zh_unwrap_kernel"]["LDS Size [bytes/block]"] == total == 4928
    m = re.search(r"kZhEncodeLds = ([\d ]+) bytes", head)
    assert usage["mi::zh_encode_kernel"]["LDS Size [bytes/block]"] == int(m.group(1).replace(" ", "")) == 5376
    assert usage["mi::zh_recode_encode_kernel"]["LDS Size [bytes/block]"] == 5376
    for name in ("mi::zh_recode_place_kernel", "mi::zh_redecode_kernel", "mi::zh_rep_rows_kernel", "mi::zh_rules_merge_kernel", "mi::zh_sources_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] == 0, name          # the recheck's decoder is the LZ4 one: no table
    hip = open(os.path.join(CSRC, "mi_zentropy.hip")).read()
    assert "zh_unwrap_kernel: 4 928 bytes" in hip and "zh_encode_kernel: 5 376 bytes" in hip


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """DESIGN 4.16's table, as compiled; every kernel but the classify pass runs at eight waves per SIMD under 64 VGPRs, the
    plan-shaped ones hold the block sums' and the scan's few words"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.16"):]
    rows = dict((m.group(1), (int(m.group(2)), int(m.group(3).replace(" ", "")))) for m in
                re.finditer(r"^\| `(zh_\w+)` \| (\d+) \| ([\d ]+) \|", section, re.M))
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds) in rows.items():
        assert (usage["mi::" + k]["VGPRs"], usage["mi::" + k]["LDS Size [bytes/block]"]) == (vgprs, lds), (k, usage["mi::" + k])
    for name in KERNELS:
        if name != "mi::zh_classify_kernel":                       # nine running sums a thread: 74 VGPRs, six waves -- one launch a call
            assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8, (name, usage[name])
    assert usage["mi::zh_classify_kernel"]["VGPRs"] <= 80 and usage["mi::zh_classify_kernel"]["Occupancy [waves/SIMD]"] >= 6
    for name in ("mi::zh_classify_kernel", "mi::zh_offsets_kernel", "mi::zh_place_kernel", "mi::zh_sources_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] <= 320, (name, usage[name])

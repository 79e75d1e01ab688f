"""What the compiler made of mi_zrecode.hip, checked without a GPU in the manner of test_kernel_resources_zprune.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["mi::zrecode_block_offsets_kernel", "mi::zrecode_block_sums_kernel", "mi::zrecode_choose_kernel", "mi::zrecode_compact_kernel",
           "mi::zrecode_decode_kernel", "mi::zrecode_encode_l1_kernel", "mi::zrecode_encode_l2_kernel", "mi::zrecode_export_kernel",
           "mi::zrecode_gather_kernel", "mi::zrecode_list_kernel", "mi::zrecode_move_offsets_kernel", "mi::zrecode_move_sums_kernel",
           "mi::zrecode_recheck_kernel", "mi::zrecode_redecode_kernel", "mi::zrecode_repoint_kernel", "mi::zrecode_stage_kernel"]
CODERS = {"mi::zrecode_encode_l1_kernel": 16384, "mi::zrecode_encode_l2_kernel": 32768}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zrecode.hip", [], str(tmp_path_factory.mktemp("kres_zrecode")))


def test_no_zrecode_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_coding_kernels_hold_the_tables_their_level_needs(usage):
    """16 KiB a wave at level 1 (one table of 4 096 positions), 32 KiB at level 2 (t4 | t8), as zpack_encode_kernel and
    zencode_l2_kernel; the workgroup is the wave"""
    for name, lds in CODERS.items():
        assert usage[name]["LDS Size [bytes/block]"] == lds, (name, usage[name])


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """everything but the two coders runs at eight waves per SIMD under 64 VGPRs; the coders are bound by their LDS
    (level 1: 55 VGPRs, level 2: 77); the gather is mi_gather.h's: 16 400 bytes of LDS; the choose kernel keeps five partial sums
    per wave, the scan's four words and the two range heads: 208 bytes; nothing else holds more than 96 bytes"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("### 4.15"):]
    for name in KERNELS:
        u = usage[name]
        if name in CODERS:
            continue
        assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] == 8, (name, u)
    assert usage["mi::zrecode_encode_l1_kernel"]["VGPRs"] <= 64 and usage["mi::zrecode_encode_l2_kernel"]["VGPRs"] <= 96
    assert usage["mi::zrecode_gather_kernel"]["LDS Size [bytes/block]"] == 16400
    assert usage["mi::zrecode_choose_kernel"]["LDS Size [bytes/block]"] == 208
    for name in KERNELS:
        if name not in CODERS and name not in ("mi::zrecode_gather_kernel", "mi::zrecode_choose_kernel"):
            assert usage[name]["LDS Size [bytes/block]"] <= 96, (name, usage[name])
    for name in ("mi::zrecode_decode_kernel", "mi::zrecode_redecode_kernel", "mi::zrecode_stage_kernel", "mi::zrecode_repoint_kernel",
                 "mi::zrecode_export_kernel", "mi::zrecode_recheck_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] == 0, name
    # the table of DESIGN 4.15: `kernel | VGPRs | LDS` rows, as compiled
    rows = dict((m.group(1), (int(m.group(2)), int(m.group(3).replace(" ", "")))) for m in
                re.finditer(r"^\| `(zrecode_\w+)` \| (\d+) \| ([\d ]+) \|", section, re.M))
    assert sorted("mi::" + k for k in rows) == KERNELS
    for k, (vgprs, lds) in rows.items():
        assert (usage["mi::" + k]["VGPRs"], usage["mi::" + k]["LDS Size [bytes/block]"]) == (vgprs, lds), (k, usage["mi::" + k])

"""What the compiler made of mi_zbatch.hip, checked without a GPU in the manner of test_kernel_resources_zset.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zbatch_block_offsets_kernel", "mi::zbatch_compact_kernel", "mi::zbatch_compare_kernel", "mi::zbatch_encode_kernel",
           "mi::zbatch_gather_kernel", "mi::zbatch_held_kernel", "mi::zbatch_layout_sums_kernel", "mi::zbatch_place_kernel",
           "mi::zbatch_plan_sums_kernel", "mi::zbatch_want_rows_kernel", "mi::zbatch_want_sums_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zbatch.hip", [], str(tmp_path_factory.mktemp("kres_zbatch")))


def test_no_zbatch_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_coder_and_the_gather_keep_the_figures_the_design_states(usage):
    """the encoder is 4.9's with another input pointer -- ONE wave a workgroup, a table of 4 096 32-bit positions =
    16 384 bytes of LDS, which the compiler states as 3 waves per SIMD, under 64 VGPRs.  The gather is its siblings' with an
    unaligned unit load: at most 16 400 bytes of LDS, at most 64 VGPRs, eight waves per SIMD."""
    enc = usage["mi::zbatch_encode_kernel"]
    assert enc["LDS Size [bytes/block]"] == 16384 and enc["Occupancy [waves/SIMD]"] == 3 and enc["VGPRs"] <= 64, enc
    g = usage["mi::zbatch_gather_kernel"]
    assert g["LDS Size [bytes/block]"] <= 16400 and g["VGPRs"] <= 64 and g["Occupancy [waves/SIMD]"] == 8, g
    for name in KERNELS:
        if name not in ("mi::zbatch_encode_kernel", "mi::zbatch_gather_kernel"):
            assert usage[name]["VGPRs"] <= 96 and usage[name]["Occupancy [waves/SIMD]"] >= 5 and usage[name]["LDS Size [bytes/block]"] <= 160, \
                (name, usage[name])

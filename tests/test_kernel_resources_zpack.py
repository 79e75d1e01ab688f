"""What the compiler made of mi_zpack.hip, checked without a GPU in the manner of test_kernel_resources_fetch.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zpack_block_offsets_kernel", "mi::zpack_block_sums_kernel", "mi::zpack_compare_kernel", "mi::zpack_decode_kernel",
           "mi::zpack_encode_kernel", "mi::zpack_gather_kernel", "mi::zpack_place_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zpack.hip", [], str(tmp_path_factory.mktemp("kres_zpack")))


def test_no_zpack_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_coder_and_the_gather_keep_the_figures_the_design_states(usage):
    """the encoder's workgroup is ONE wave with a table of 4 096 32-bit positions = 16 384 bytes of LDS; ten such
    workgroups fit a CU's 160 KiB, which the compiler states as 3 waves per SIMD (the tenth workgroup rounds 2.5 up), and its
    registers (under 64) would allow eight.  The decoder keeps nothing in LDS and runs at eight waves per SIMD.  The gather is
    mi_fetch.hip's: 16 400 bytes, eight waves."""
    enc = usage["mi::zpack_encode_kernel"]
    assert enc["LDS Size [bytes/block]"] == 16384 and enc["Occupancy [waves/SIMD]"] == 3 and enc["VGPRs"] <= 64, enc
    dec = usage["mi::zpack_decode_kernel"]
    assert dec["LDS Size [bytes/block]"] == 0 and dec["Occupancy [waves/SIMD]"] == 8 and dec["VGPRs"] <= 64, dec
    g = usage["mi::zpack_gather_kernel"]
    assert g["LDS Size [bytes/block]"] == 16400 and g["VGPRs"] <= 64 and g["Occupancy [waves/SIMD]"] == 8, g
    for name in ("mi::zpack_block_offsets_kernel", "mi::zpack_block_sums_kernel", "mi::zpack_compare_kernel", "mi::zpack_place_kernel"):
        assert usage[name]["VGPRs"] <= 96 and usage[name]["Occupancy [waves/SIMD]"] >= 5 and usage[name]["LDS Size [bytes/block]"] <= 128, (name, usage[name])

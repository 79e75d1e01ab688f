"""What the compiler made of mi_zpack2.hip, checked without a GPU in the manner of test_kernel_resources_zpack.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zencode_l2_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zpack2.hip", [], str(tmp_path_factory.mktemp("kres_zpack2")))


def test_the_level_2_coder_does_not_spill_and_its_lds_is_exactly_the_two_tables(usage):
    """ONE wave a workgroup with two tables of 4 096 32-bit positions = 32 768 bytes of LDS and nothing else; five
    such workgroups fit a CU's 160 KiB, which the compiler states as 2 waves per SIMD (level 1: ten workgroups, 3).  No scratch:
    the lanes' private length loops keep their state in registers, under 128."""
    assert sorted(usage) == KERNELS, sorted(usage)
    enc = usage["mi::zencode_l2_kernel"]
    assert enc["ScratchSize [bytes/lane]"] == 0 and enc["VGPRs Spill"] == 0 and enc["SGPRs Spill"] == 0 and enc["AGPRs"] == 0, enc
    assert enc["LDS Size [bytes/block]"] == 2 * 4096 * 4 and enc["Occupancy [waves/SIMD]"] == 2 and enc["VGPRs"] <= 128, enc


def test_the_level_1_coders_are_not_rebuilt_around_a_level():
    """the level is chosen on the host between two launches: mi_zpack.hip and mi_zbatch.hip do not include the level-2 coder, so
    their kernels compile from what they compiled from before (test_kernel_resources_zpack.py and _zbatch.py hold their figures)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "makisu_amd", "csrc")
    for name in ("mi_zpack.hip", "mi_zbatch.hip", "mi_lz4_wave_enc.h"):
        assert "mi_lz4_wave_enc2.h" not in open(os.path.join(csrc, name)).read(), name

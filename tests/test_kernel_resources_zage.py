"""What the compiler made of mi_zage.hip, checked without a GPU in the manner of test_kernel_resources_zprune.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zage_carry_kernel", "mi::zage_census_kernel", "mi::zage_mark_kernel", "mi::zage_stamps_kernel", "mi::zage_touch_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zage.hip", [], str(tmp_path_factory.mktemp("kres_zage")))


def test_exactly_the_five_kernels_and_none_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """every kernel runs at eight waves per SIMD under 64 VGPRs; the census holds its bins in LDS -- 256 bins of four
    64-bit values and 256 bounds: 9 216 bytes; nothing else holds more than 64 bytes."""
    for name in KERNELS:
        assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8, (name, usage[name])
    assert usage["mi::zage_census_kernel"]["LDS Size [bytes/block]"] == 256 * 4 * 8 + 256 * 4
    for name in KERNELS:
        if name != "mi::zage_census_kernel":
            assert usage[name]["LDS Size [bytes/block]"] <= 64, (name, usage[name])

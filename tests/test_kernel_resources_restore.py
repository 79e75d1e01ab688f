"""What the compiler made of mi_restore.hip, checked without a GPU in the manner of test_kernel_resources_pack.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::packset_check_kernel", "mi::packset_unpack_kernel", "mi::restore_assemble_kernel", "mi::restore_compare_kernel",
           "mi::restore_lookup_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_restore.hip", [], str(tmp_path_factory.mktemp("kres_restore")))


def test_no_restore_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_assemble_kernel_keeps_the_figures_the_design_states(usage):
    """a 256-thread workgroup writes a 16 KiB tile; up to 1 024 of the tile's rows lie in LDS -- destination offset
    8, source address 8 and length 4 bytes each, two words for the search and the joined-unit counter = 20 504 bytes, seven
    workgroups per CU by LDS; four 16-byte loads in flight per lane with their addresses, lengths and rows take just over 64
    VGPRs (72 are allocated at most), which allows the same seven waves per SIMD."""
    g = usage["mi::restore_assemble_kernel"]
    assert g["LDS Size [bytes/block]"] == 20504, g
    assert g["VGPRs"] <= 72 and g["Occupancy [waves/SIMD]"] == 7, g
    for name in KERNELS:
        if name != "mi::restore_assemble_kernel":
            # the set's, the lookup and the compare kernels: a counter word in LDS at the most
            assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8 and usage[name]["LDS Size [bytes/block]"] <= 16, (name, usage[name])

"""What the compiler made of mi_pack.hip, checked without a GPU in the manner of test_kernel_resources_blake2s.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::pack_block_offsets_kernel", "mi::pack_block_sums_kernel", "mi::pack_compact_kernel", "mi::pack_compare_kernel",
           "mi::pack_gather_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_pack.hip", [], str(tmp_path_factory.mktemp("kres_pack")))


def test_no_pack_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_gather_kernel_keeps_the_figures_the_design_states(usage):
    """a 256-thread workgroup writes a 16 KiB tile; the tile's entries lie in LDS -- at most 1 024 of them (an
    entry takes a 16-byte unit at least): 8 + 4 + 4 bytes each and two words for the search = 16 400 bytes, nine workgroups
    per CU by LDS; four 16-byte loads in flight per lane and their addresses and lengths fit 64 VGPRs, so the registers
    allow the full eight waves per SIMD."""
    g = usage["mi::pack_gather_kernel"]
    assert g["LDS Size [bytes/block]"] == 16400, g
    assert g["VGPRs"] <= 64 and g["Occupancy [waves/SIMD]"] == 8, g
    for name in KERNELS:
        if name != "mi::pack_gather_kernel":
            # the plan kernels: four u64 for the scans' wave totals; the block sums reduce three values in one go (3 x 4 u64)
            assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8 and usage[name]["LDS Size [bytes/block]"] <= 96, (name, usage[name])

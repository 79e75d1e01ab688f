"""What the compiler made of mi_fetch.hip, checked without a GPU in the manner of test_kernel_resources_restore.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::fetch_block_offsets_kernel", "mi::fetch_block_sums_kernel", "mi::fetch_compact_entries_kernel",
           "mi::fetch_compact_rows_kernel", "mi::fetch_compare_kernel", "mi::fetch_gather_kernel", "mi::fetch_lookup_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_fetch.hip", [], str(tmp_path_factory.mktemp("kres_fetch")))


def test_no_fetch_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_gather_kernel_keeps_the_figures_the_design_states(usage):
    """a 256-thread workgroup writes a 16 KiB tile; the tile's entries lie in LDS -- at most 1 024 of them (an
    entry takes a 16-byte unit at least): source address 8, place in the tile 4 and length 4 bytes each and two words for the
    search = 16 400 bytes, nine workgroups per CU by LDS; four 16-byte loads in flight per lane and their addresses and
    lengths fit 64 VGPRs, so the registers allow the full eight waves per SIMD."""
    g = usage["mi::fetch_gather_kernel"]
    assert g["LDS Size [bytes/block]"] == 16400, g
    assert g["VGPRs"] <= 64 and g["Occupancy [waves/SIMD]"] == 8, g
    for name in KERNELS:
        if name != "mi::fetch_gather_kernel":
            # the lookup, the plan and the compare kernels: four u64 for the scans' wave totals; the block sums reduce six
            # values in one go (6 x 4 u64)
            assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8 and usage[name]["LDS Size [bytes/block]"] <= 192, (name, usage[name])

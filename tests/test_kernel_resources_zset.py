"""What the compiler made of mi_zset.hip, checked without a GPU in the manner of test_kernel_resources_zpack.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zset_block_offsets_kernel", "mi::zset_block_sums_kernel", "mi::zset_compact_entries_kernel", "mi::zset_compare_kernel",
           "mi::zset_gather_kernel", "mi::zset_lookup_kernel", "mi::zset_restore_kernel", "mi::zset_unpack_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zset.hip", [], str(tmp_path_factory.mktemp("kres_zset")))


def test_no_zset_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_fused_restore_and_the_gather_keep_the_figures_the_design_states(usage):
    """the fused restore's workgroup is one wave that keeps nothing in LDS -- the decoder of mi_lz4_wave.h plus a
    copy loop -- and stays under 64 VGPRs, eight waves per SIMD; the gather is mi_zpack.hip's: 16 400 bytes of LDS."""
    r = usage["mi::zset_restore_kernel"]
    assert r["LDS Size [bytes/block]"] == 0 and r["VGPRs"] <= 64 and r["Occupancy [waves/SIMD]"] == 8, r
    g = usage["mi::zset_gather_kernel"]
    assert g["LDS Size [bytes/block]"] <= 16400 and g["VGPRs"] <= 64 and g["Occupancy [waves/SIMD]"] == 8, g
    for name in KERNELS:
        if name not in ("mi::zset_restore_kernel", "mi::zset_gather_kernel"):
            assert usage[name]["VGPRs"] <= 96 and usage[name]["Occupancy [waves/SIMD]"] >= 5 and usage[name]["LDS Size [bytes/block]"] <= 160, \
                (name, usage[name])

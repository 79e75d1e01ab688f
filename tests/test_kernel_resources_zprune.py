"""What the compiler made of mi_zprune.hip, checked without a GPU in the manner of test_kernel_resources_zset.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::zprune_block_offsets_kernel", "mi::zprune_block_sums_kernel", "mi::zprune_compact_kernel", "mi::zprune_export_kernel",
           "mi::zprune_gather_kernel", "mi::zprune_live_kernel", "mi::zprune_mark_kernel", "mi::zprune_repoint_kernel",
           "mi::zprune_sweep_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_zprune.hip", [], str(tmp_path_factory.mktemp("kres_zprune")))


def test_no_zprune_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """every kernel runs at eight waves per SIMD under 64 VGPRs; the move is zset_gather_kernel's: 16 400 bytes of
    LDS (three arrays of 1 024 spans and two words); the sweep keeps 256 per-blob bins and four partial sums per wave: 2 176
    bytes; nothing else holds more than 64 bytes."""
    for name in KERNELS:
        assert usage[name]["VGPRs"] <= 64 and usage[name]["Occupancy [waves/SIMD]"] == 8, (name, usage[name])
    assert usage["mi::zprune_gather_kernel"]["LDS Size [bytes/block]"] == 16400
    assert usage["mi::zprune_sweep_kernel"]["LDS Size [bytes/block]"] == 2176
    for name in KERNELS:
        if name not in ("mi::zprune_gather_kernel", "mi::zprune_sweep_kernel"):
            assert usage[name]["LDS Size [bytes/block]"] <= 64, (name, usage[name])
    for name in ("mi::zprune_mark_kernel", "mi::zprune_repoint_kernel", "mi::zprune_export_kernel"):
        assert usage[name]["LDS Size [bytes/block]"] == 0, name

"""What the compiler made of mi_slot_table.hip -- the pack sets' digest table, plain and compressed -- checked without a GPU in
the manner of test_kernel_resources_zset.py: registers, spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage
(DESIGN.md 4.7, 4.10)."""
import os

import pytest

from test_kernel_resources import HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

KERNELS = ["mi::slot_table_begin_kernel", "mi::slot_table_export_kernel", "mi::slot_table_probe_kernel<false>",
           "mi::slot_table_probe_kernel<true>", "mi::slot_table_verify_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("mi_slot_table.hip", [], str(tmp_path_factory.mktemp("kres_slot_table")))


def test_no_slot_table_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == KERNELS, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_table_kernels_keep_the_figures_of_a_set_s_ordinary_kernels(usage):
    """The probe kernel -- with a compressed set's two byte sums and without -- keeps three counter words in LDS, the others nothing."""
    for name in KERNELS:
        assert usage[name]["VGPRs"] <= 96 and usage[name]["Occupancy [waves/SIMD]"] >= 5 and usage[name]["LDS Size [bytes/block]"] <= 160, \
            (name, usage[name])

"""What the compiler made of mi_index.hip, checked without a GPU in the manner of test_kernel_resources_zprune.py: registers,
spills, scratch and LDS from -Rpass-analysis=kernel-resource-usage.  The file's kernels live in an anonymous
namespace, which test_kernel_resources._usage's name parsing folds into one empty name, so the remarks are read here."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

OLD = ["index_begin_kernel", "index_export_kernel", "index_inherit_kernel", "index_probe_kernel", "index_verify_kernel"]
NEW = ["index_held_flags_kernel", "index_lookup_kernel", "index_sweep_kernel"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("kres_index"))
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mi_index.hip"), "-o", os.path.join(tmp, "dev.o")],
                         capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            cur = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "").split("(")[0]
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*?): (\d+) \[-Rpass", line)
        if m and cur:
            kernels[cur][m.group(1).strip()] = int(m.group(2))
    return kernels


def test_the_kernels_are_the_five_old_ones_and_the_three_new_and_none_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == sorted(OLD + NEW), sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_the_kernels_keep_the_figures_the_design_states(usage):
    """every kernel of the file runs at eight waves per SIMD; the lookup holds two digests' words and its walk in 30
    VGPRs, the sweep 12, the flags kernel 4; none of the new ones uses LDS (their sums go through ballots: one atomic a wave)."""
    for name in OLD + NEW:
        assert usage[name]["Occupancy [waves/SIMD]"] == 8 and usage[name]["VGPRs"] <= 64, (name, usage[name])
    assert [usage[n]["VGPRs"] for n in NEW] == [4, 30, 12], [usage[n] for n in NEW]
    for name in NEW:
        assert usage[name]["LDS Size [bytes/block]"] == 0, (name, usage[name])

"""What the compiler made of blake2s.hip, checked without a GPU in the manner of test_kernel_resources.py: registers, spills,
scratch and LDS from -Rpass-analysis=kernel-resource-usage, and the instruction mix of the compression from the disassembly
(DESIGN.md 4.2b)."""
import collections
import os
import re
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, _usage

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
EXTRA = ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    return _usage("blake2s.hip", EXTRA, str(tmp_path_factory.mktemp("kres_b2s")))


def test_no_blake2s_kernel_spills_or_uses_scratch_or_agprs(usage):
    assert sorted(usage) == ["mi::blake2s_items_kernel<0, false>", "mi::blake2s_items_kernel<0, true>",
                             "mi::blake2s_items_kernel<1, false>", "mi::blake2s_roof_kernel"], sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["AGPRs"] == 0, (name, u)


def test_blake2s_kernels_keep_their_occupancy_step(usage):
    """The launch geometry is the SHA pass's: two 256-thread workgroups per CU pinned by LDS for the lane-owned
    loads, three from 24 GiB on for the cooperative ones, and the chunk pass of ANOTHER batch in flight must fit beside them:
    four waves per SIMD = 128 of the 512 VGPRs per lane.  That is the step: the lane-owned form (8 state + 16 message + 16
    working words + 32 words of loads in flight + the queue bookkeeping) sits below 128 -> 4 waves per SIMD, the
    cooperative form carries 16 more words in flight and its 20 KiB of LDS staging and must stay at 128 too."""
    for name, u in usage.items():
        if "items_kernel" not in name:
            continue
        coop = name.endswith(", true>")
        assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, (name, u)
        assert u["LDS Size [bytes/block]"] == (20480 if coop else 0), (name, u)
        # the figures any fold of this loop with sha256.hip's has to keep: not a register more
        assert u["VGPRs"] <= (122 if coop else 95), (name, u)
    assert usage["mi::blake2s_roof_kernel"]["Occupancy [waves/SIMD]"] == 8           # the roof is measured at up to 8 waves per SIMD


def _mixes(tmp_path):
    obj, co = str(tmp_path / "b2s.o"), str(tmp_path / "b2s.co")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "--cuda-device-only"] + EXTRA +
                   ["-c", os.path.join(CSRC, "blake2s.hip"), "-o", obj], check=True)
    llvm = "/opt/rocm/lib/llvm/bin/"
    subprocess.run([llvm + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + obj,
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
    asm = subprocess.run([llvm + "llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    mix = {}
    for f in re.split(r"\n(?=[0-9a-f]+ <)", asm):
        m = re.match(r"[0-9a-f]+ <(\S+)>:", f)
        if m:
            # what a wave can execute: up to the LAST s_endpgm (behind it the assembler pads the code object with s_nop)
            body, _, pad = f.rpartition("s_endpgm")
            mix[m.group(1)] = (collections.Counter(mm.group(1) for mm in re.finditer(r"^\s+([vs]_\w+)", body, re.M)),
                               len(re.findall(r"\bs_nop\b", pad)), len(re.findall(r"s_waitcnt[^\n/]*vmcnt", body)))
    return mix


def test_blake2s_instruction_count_is_at_its_floor(tmp_path):
    """DESIGN 4.2b.  The compression's floor: 80 G functions x 12 (2 v_add3_u32 + 2 v_add_u32 + 4 v_xor_b32 + 4 v_alignbit_b32)
    + 3 (t0, t1 and the final flag into v12..v14) + 8 (h ^= v[i] ^ v[i + 8], one v_bitop3_b32 each where RFC 7693 writes two
    xors: 8 below the 16 of the plain form) = 971.
    The roof kernel is the compression + its benchmark loop: 16 message words x (multiply-add of the generator + xor with the
    state: 3) + the flag, the counter and the loop = 1 035 as compiled.
    The chunk pass is the compression + one iteration of the loop: the 16-word copy out of the load registers (the next
    block's loads are already in flight into them), the tail's zero fill (16 words x 4), the stage machine of the next-string
    pipeline, the dequeue and the store = 1 222 as compiled (the cooperative form: 1 286 with its 16 v_perm_b32 and the
    quad broadcasts)."""
    mix = _mixes(tmp_path)
    roof, roof_pad, _ = next(v for k, v in mix.items() if "blake2s_roof_kernel" in k)
    chunk, _, _ = next(v for k, v in mix.items() if "blake2s_items_kernelILi0ELb0E" in k)
    coop, _, _ = next(v for k, v in mix.items() if "blake2s_items_kernelILi0ELb1E" in k)
    valu = lambda c: sum(n for k, n in c.items() if k.startswith("v_"))                                   # noqa: E731
    for c in (roof, chunk, coop):
        assert c["v_alignbit_b32"] == 320 and c["v_add3_u32"] >= 160 and c["v_add3_u32"] <= 164, c
        assert c["v_bitop3_b32"] == 8
    assert valu(roof) <= 1040, valu(roof)                          # 1 035
    assert valu(chunk) <= 1235, valu(chunk)                        # 1 222
    assert valu(coop) <= 1300, valu(coop)                          # 1 286
    assert valu(chunk) <= 1222 and valu(coop) <= 1286              # ... nor an instruction
    assert coop["v_perm_b32"] == 16 and chunk["v_perm_b32"] == 0   # the realignment; lane-owned loads ARE the message words
    # s_waitcnt instructions that name vmcnt: three per item kernel, one of them the loop top's own -- one more is a wait on
    # memory that hipcc has put somewhere in the iteration
    waits = {k: v[2] for k, v in mix.items() if "blake2s_items_kernel" in k}
    assert len(waits) == 3 and set(waits.values()) == {3}, waits
    # s_nop.  The 250-odd of a plain compile of the compression are NOT hazard pads: they stand behind s_endpgm, where the
    # assembler fills the code object up to its alignment, and no wave reaches them.  The compression itself has none ...
    assert roof["s_nop"] == 0 and roof_pad >= 1, (roof["s_nop"], roof_pad)
    # ... and the loop's are the wait states between a v_cmp that writes VCC and the v_cndmask that reads it, in the tail's
    # zero fill (16 as compiled: one per word; 18 in the cooperative form), which runs once per string, not per block
    assert chunk["s_nop"] <= 16 and coop["s_nop"] <= 18, (chunk["s_nop"], coop["s_nop"])

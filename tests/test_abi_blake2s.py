"""The ABI side of MI_FLAG_CHUNK_BLAKE2S: additions only -- a flag bit, two constants, three prototypes under the MI_BLOCK /
MI_DIAG banners (the core shim set does not grow) -- at ABI version 6, and a default config that does not set the flag."""
import ctypes as C
import os
import re

import makisu_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "makisu_mi.h")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_the_flag_and_the_three_exports_are_in_the_header_each_with_one_tag(engine_lib):
    src = _header()
    assert re.search(r"^#define\s+MI_FLAG_CHUNK_BLAKE2S\s+0x40u\b", src, re.M)
    assert re.search(r"^#define\s+MI_DIGEST_SHA256\s+0u?\b", src, re.M) and re.search(r"^#define\s+MI_DIGEST_BLAKE2S\s+1u?\b", src, re.M)
    flags = {n: int(v, 16) for n, v in re.findall(r"^#define\s+(MI_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", src, re.M)}
    assert [n for n, v in flags.items() if v == 0x40] == ["MI_FLAG_CHUNK_BLAKE2S"]           # the bit the issue names, taken once
    for name, tag in (("mi_ctx_chunk_digest", "MI_BLOCK"), ("mi_chunk_root_alg", "MI_BLOCK"), ("mi_blake2s_valu_roof", "MI_DIAG")):
        tags = re.findall(r"^(MI_CORE|MI_BLOCK|MI_DIAG)\s[^\n(;]*?\b%s\s*\(" % name, src, re.M)
        assert tags == [tag], (name, tags)
        assert len(re.findall(r"\b%s\s*\(" % name, src)) == 1, name
        assert hasattr(engine_lib, name) and name in engine_lib._mi_symbols
    assert re.search(r"int\s+mi_ctx_chunk_digest\(mi_ctx\*\s*\w+,\s*uint32_t\*\s*\w+\)", src)
    assert re.search(r"int\s+mi_chunk_root_alg\(uint32_t\s+\w+,\s*const uint8_t\*\s*\w+,\s*uint64_t\s+\w+,\s*uint8_t\*\s*\w+\)", src)
    assert re.search(r"int\s+mi_blake2s_valu_roof\(mi_ctx\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*double\*\s*\w+\)", src)
    assert re.search(r"int\s+mi_chunk_root\(const uint8_t\*\s*\w+,\s*uint64_t\s+\w+,\s*uint8_t\*\s*\w+\)", src)   # unchanged


def test_the_abi_version_stays_6_and_the_default_leaves_the_flag_clear(engine_lib):
    assert engine_lib.mi_abi_version() == 6
    assert re.search(r"^#define\s+MI_ABI_VERSION\s+6\b", open(HEADER).read(), re.M)
    cfg = makisu_amd.default_config()
    assert cfg.flags == 0 and not cfg.flags & makisu_amd.FLAG_CHUNK_BLAKE2S
    assert cfg.struct_size == C.sizeof(makisu_amd.Config)
    assert makisu_amd.default_config(flags=makisu_amd.FLAG_CHUNK_BLAKE2S).flags == 0x40


def test_the_python_names():
    assert (makisu_amd.FLAG_CHUNK_BLAKE2S, makisu_amd.DIGEST_SHA256, makisu_amd.DIGEST_BLAKE2S) == (0x40, 0, 1)
    assert isinstance(makisu_amd.Engine.chunk_digest, property) and callable(makisu_amd.Engine.blake2s_valu_roof)
    for n in ("FLAG_CHUNK_BLAKE2S", "DIGEST_SHA256", "DIGEST_BLAKE2S", "chunk_root"):
        assert n in makisu_amd.__all__


def test_null_arguments_are_refused(engine_lib):
    assert engine_lib.mi_ctx_chunk_digest(None, C.byref(C.c_uint32())) == -1
    assert engine_lib.mi_blake2s_valu_roof(None, 0, 0, C.byref(C.c_double())) == -1
    assert engine_lib.mi_chunk_root_alg(1, None, 1, (C.c_uint8 * 32)()) == -1
    assert engine_lib.mi_chunk_root_alg(1, None, 0, None) == -1

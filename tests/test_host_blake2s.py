"""BLAKE2s-256 on the host (csrc/host_blake2s.h) and the chunk root built with it (mi_chunk_root_alg), against hashlib -- a
reference nobody here wrote.  No GPU: the root function and the hasher are host code."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import makisu_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "makisu_amd", "csrc")


def tree_model(digests, hash_fn):
    """the fan-out-64 tree of include/makisu_mi.h (mi_chunk_root_alg): one hash over at most 64 digests put end to end,
    levels of 64 above that"""
    nodes = [bytes(d) for d in digests]
    while len(nodes) > 64:
        nodes = [hash_fn(b"".join(nodes[i:i + 64])).digest() for i in range(0, len(nodes), 64)]
    return hash_fn(b"".join(nodes)).digest()


NS = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 64 ** 3 + 1]


@pytest.mark.parametrize("n", NS)
def test_blake2s_chunk_root_is_the_tree_with_blake2s_at_every_node(n):
    d = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    assert makisu_amd.chunk_root(d, alg=makisu_amd.DIGEST_BLAKE2S) == tree_model(d, hashlib.blake2s)


@pytest.mark.parametrize("n", NS)
def test_sha256_alg_is_todays_chunk_root(n, engine_lib):
    d = np.random.default_rng(1000 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    today = np.zeros(32, dtype=np.uint8)
    assert engine_lib.mi_chunk_root(d.ctypes.data if n else None, n, today.ctypes.data) == 0
    assert makisu_amd.chunk_root(d, alg=makisu_amd.DIGEST_SHA256) == today.tobytes() == makisu_amd.chunk_root(d)
    assert today.tobytes() == tree_model(d, hashlib.sha256)
    assert n == 0 or makisu_amd.chunk_root(d, alg=makisu_amd.DIGEST_BLAKE2S) != today.tobytes()


def test_an_unknown_algorithm_is_refused():
    with pytest.raises(makisu_amd.MiError) as ei:
        makisu_amd.chunk_root(np.zeros((1, 32), np.uint8), alg=2)
    assert ei.value.code == -1


DRIVER = r'''
#include <stdio.h>
#include <vector>
#include "host_blake2s.h"
static void put(const uint8_t* d) { for (int i = 0; i < 32; ++i) printf("%02x", d[i]); printf("\n"); }
int main() {
    uint8_t out[32];
    for (size_t n = 0; n <= 300; ++n) {
        std::vector<uint8_t> b(n + 1);
        for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)(i * 7 + n * 13 + 3);
        mi_host::Blake2s whole;
        whole.update(b.data(), n);
        whole.final(out);
        put(out);
        mi_host::Blake2s pieces;                       // uneven pieces: 1, 2, 3, ... bytes, an empty one in between
        size_t at = 0, step = 1;
        while (at < n) {
            const size_t take = step < n - at ? step : n - at;
            pieces.update(b.data() + at, take);
            pieces.update(b.data() + at, 0);
            at += take;
            step = step % 67 + 1 + (at % 5);
        }
        pieces.final(out);
        put(out);
        pieces.reset();                                // ... and an object that is used again
        pieces.update(b.data(), n / 2);
        pieces.update(b.data() + n / 2, n - n / 2);
        pieces.final(out);
        put(out);
    }
    mi_host::Blake2s abc;
    abc.update("abc", 3);
    abc.final(out);
    put(out);
    return 0;
}
'''


def test_the_host_hasher_is_hashlibs_blake2s(tmp_path):
    """every length 0..300 (the block boundaries 64, 128, 192, 256 and both sides of each), whole, in uneven pieces and
    on a reused object; RFC 7693 appendix B's "abc" """
    src, exe = tmp_path / "b2s.cpp", tmp_path / "b2s"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().split()
    assert len(lines) == 3 * 301 + 1
    for n in range(301):
        want = hashlib.blake2s(bytes((i * 7 + n * 13 + 3) & 0xFF for i in range(n))).hexdigest()
        assert lines[3 * n: 3 * n + 3] == [want] * 3, n
    rfc = "508c5e8c327c14e2e1a72ba34eeb452f37458b209ed63a294d999b4c86675982"
    assert lines[-1] == rfc == hashlib.blake2s(b"abc").hexdigest()


# ---- the kernel's own device functions, compiled for the host -------------------------------------------------------
LANE_SHIM = r'''
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef uint8_t u8; typedef uint32_t u32; typedef uint64_t u64;
#define __device__
#define __forceinline__ inline
struct u32x4 { u32 x, y, z, w; };
static inline u32 __builtin_amdgcn_alignbit(u32 a, u32 b, u32 n) { return (u32)(((((u64)a) << 32) | b) >> (n & 31)); }
static inline u32 __builtin_amdgcn_bitop3_b32(u32 a, u32 b, u32 c, int tt) { u32 r = 0; for (int i = 0; i < 32; ++i) { int idx = (((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1); r |= (u32)((tt >> idx) & 1) << i; } return r; }
static inline u32 __builtin_amdgcn_perm(u32 hi, u32 lo, u32 sel) { u64 p = ((u64)hi << 32) | lo; u32 r = 0; for (int i = 0; i < 4; ++i) { u32 b = (sel >> (8 * i)) & 0xFF; r |= (u32)((p >> (8 * b)) & 0xFF) << (8 * i); } return r; }
'''
LANE_LOOP = r'''
static u32x4 ld(const u8* p) { u32x4 v; memcpy(&v, p, 16); return v; }
// one lane of blake2s_items_kernel, lane-owned or cooperative window
static void hash_string(const u8* base, u64 off, u64 len, bool coop, u8* out) {
    const u8* p = base + off; const u8* ptr; u32 sel = 0x03020100u, carry = 0;
    u32x4 nx0{}, nx1{}, nx2{}, nx3{};
    if (coop) { const u32 mis = (u32)(size_t)p & 3u; const u8* q = p - mis; ptr = q + 4; sel = 0x03020100u + mis * 0x01010101u;
        if (len) { memcpy(&carry, q, 4); nx0 = ld(q + 4); nx1 = ld(q + 20); nx2 = ld(q + 36); nx3 = ld(q + 52); } }
    else { ptr = p; if (len) { nx0 = ld(p); nx1 = ld(p + 16); nx2 = ld(p + 32); nx3 = ld(p + 48); } }
    u64 rem = len, total = len; u32 h[8]; blake2s_iv(h);
    for (;;) {
        u32 m[16]; bool last = false;
        if (coop) block_words_coop(m, nx0, nx1, nx2, nx3, carry, sel); else block_words_lane(m, nx0, nx1, nx2, nx3);
        if (rem > 64) { ptr += 64; rem -= 64; nx0 = ld(ptr); nx1 = ld(ptr + 16); nx2 = ld(ptr + 32); nx3 = ld(ptr + 48); }
        else { if (rem < 64) zero_tail(m, (u32)rem); rem = 0; last = true; }
        blake2s_compress(h, m, total - rem, last);
        if (last) break;
    }
    memcpy(out, h, 32);
}
int main(int, char** argv) {
    std::vector<u8> buf(1 << 20); u32 x = 12345; for (auto& b : buf) { x = x * 1664525u + 1013904223u; b = (u8)(x >> 24); }
    fwrite(buf.data(), 1, buf.size(), fopen(argv[1], "wb"));
    for (u64 len = 0; len <= 600; ++len) for (u64 off = 16; off < 24; ++off) for (int coop = 0; coop < 2; ++coop) {
        u8 d[32]; hash_string(buf.data(), off + len * 3, len, coop, d);
        printf("%llu %llu %d ", (unsigned long long)(off + len * 3), (unsigned long long)len, coop); for (int i = 0; i < 32; ++i) printf("%02x", d[i]); printf("\n"); }
    u8 d[32]; hash_string(buf.data(), 4099, 70001, true, d); printf("4099 70001 1 "); for (int i = 0; i < 32; ++i) printf("%02x", d[i]); printf("\n");
    return 0;
}
'''


def test_one_lane_of_the_kernel_on_the_host(tmp_path):
    """blake2s.hip's device functions as they stand in the file (everything in its unnamed namespace: the compression, the
    tail's zero fill, the message words of both load schemes, the IV) compiled for the host behind three shims for the gfx950
    builtins, and driven the way a lane of blake2s_items_kernel drives them -- the block that ends the string is the last one,
    also at a multiple of 64; t counts bytes; the cooperative window starts at the dword below the string: every length
    0..600 at every byte alignment, both schemes, against hashlib.  What the GPU adds is the loop around it (queues, loads in
    flight), which tests/test_gpu_blake2s.py covers."""
    s = open(os.path.join(CSRC, "blake2s.hip")).read()
    core = s[s.index("namespace {") + len("namespace {"): s.index("}  // namespace\n")].replace("__device__ constexpr", "constexpr")
    src, exe, blob = tmp_path / "lane.cpp", tmp_path / "lane", tmp_path / "buf.bin"
    src.write_text(LANE_SHIM + core + LANE_LOOP)
    subprocess.check_call(["g++", "-O1", "-std=c++17", str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe), str(blob)]).decode().splitlines()
    buf = blob.read_bytes()
    assert len(lines) == 601 * 8 * 2 + 1
    for ln in lines:
        off, n, coop, hx = ln.split()
        assert hashlib.blake2s(buf[int(off): int(off) + int(n)]).hexdigest() == hx, (off, n, coop)

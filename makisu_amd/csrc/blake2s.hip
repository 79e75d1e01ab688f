// blake2s.hip -- batched BLAKE2s-256 (RFC 7693) on gfx950: one lane per independent byte string.
//
// The chunk digest of a ctx created with MI_FLAG_CHUNK_BLAKE2S (include/makisu_mi.h): unkeyed, no salt, no
// personalisation, sequential mode -- hashlib.blake2s(b).digest().  Chunk digests and chunk roots are this
// engine's own keys (dedup, the chunk index, "did the content change"), nothing Docker sees, so a ctx may
// trade SHA-256 for a hash with fewer instructions per block: 80 G functions of 12 VALU ops against
// SHA-256's 64 rounds of 17 + 48 schedule words of 6 (DESIGN.md 4.2b has the counts and what was measured).
//
// A sibling of sha256.hip, not a parameter of it: the loop below is that file's loop -- LPT queues with the
// wave-aggregated hand-issued dequeue, the four-stage next-string pipeline, the per-SIMD roles, both load
// schemes; sha256.hip says why each is the way it is and this file does not repeat it -- but what differs sits
// in the middle of every iteration: little-endian words (lane-owned loads ARE the message words), no padding
// block and so no pad_block state (the last block is known BEFORE it is compressed: it is the one that ends
// the string, also when the length is a multiple of 64), a byte counter and a final flag going into the
// compression.  One loop over a hash trait would have had to branch on its caller in each of those places,
// and sha256_items_kernel's compiled form, which three pull requests could not improve, would have moved.
// What the two share without a branch -- the load types, the quad fetch, kLook -- is in mi_item_loads.h.
#include "mi_common.h"
#include "mi_item_loads.h"
#include "mi_item_launch.h"

namespace mi {

namespace {

__device__ __forceinline__ u32 rotr(u32 x, u32 n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ u32 xor3(u32 a, u32 b, u32 c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }

constexpr u32 kIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
// the parameter block's first word: digest_length 32, no key, fanout 1, depth 1 (RFC 7693 2.5); the rest is zero
constexpr u32 kParam0 = 0x01010020u;
__device__ constexpr u8 kSigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

// 12 VALU ops: 2 v_add3_u32, 2 v_add_u32, 4 v_xor_b32, 4 v_alignbit_b32
__device__ __forceinline__ void blake2s_g(u32& a, u32& b, u32& c, u32& d, u32 x, u32 y) {
    a = a + b + x; d = rotr(d ^ a, 16); c += d; b = rotr(b ^ c, 12);
    a = a + b + y; d = rotr(d ^ a, 8);  c += d; b = rotr(b ^ c, 7);
}

// One compression: h = F(h, m, t, last).  The ten rounds are fully unrolled, so v[] lives in fixed VGPRs and
// sigma only picks WHICH register of m[] an add reads: no message word moves.  t = bytes hashed up to and
// including this block.
__device__ __forceinline__ void blake2s_compress(u32 (&h)[8], const u32 (&m)[16], u64 t, bool last) {
    u32 v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = h[i];
    v[8] = kIV[0]; v[9] = kIV[1]; v[10] = kIV[2]; v[11] = kIV[3];
    v[12] = kIV[4] ^ (u32)t;
    v[13] = kIV[5] ^ (u32)(t >> 32);
    v[14] = last ? ~kIV[6] : kIV[6];
    v[15] = kIV[7];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        blake2s_g(v[0], v[4], v[8],  v[12], m[kSigma[r][0]],  m[kSigma[r][1]]);
        blake2s_g(v[1], v[5], v[9],  v[13], m[kSigma[r][2]],  m[kSigma[r][3]]);
        blake2s_g(v[2], v[6], v[10], v[14], m[kSigma[r][4]],  m[kSigma[r][5]]);
        blake2s_g(v[3], v[7], v[11], v[15], m[kSigma[r][6]],  m[kSigma[r][7]]);
        blake2s_g(v[0], v[5], v[10], v[15], m[kSigma[r][8]],  m[kSigma[r][9]]);
        blake2s_g(v[1], v[6], v[11], v[12], m[kSigma[r][10]], m[kSigma[r][11]]);
        blake2s_g(v[2], v[7], v[8],  v[13], m[kSigma[r][12]], m[kSigma[r][13]]);
        blake2s_g(v[3], v[4], v[9],  v[14], m[kSigma[r][14]], m[kSigma[r][15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = xor3(h[i], v[i], v[i + 8]);    // (one v_bitop3_b32 for RFC 7693's two xors)
}

__device__ __forceinline__ void blake2s_iv(u32 (&h)[8]) {
    h[0] = kIV[0] ^ kParam0;
#pragma unroll
    for (int i = 1; i < 8; ++i) h[i] = kIV[i];
}

// The little-endian words of a 64-byte load become the last block of a string that has r (< 64) bytes left:
// the data bytes, then zeros.  Pure register work: one mask per word from its neighbour's (hipcc makes a v_cmp +
// v_cndmask of each, two wait states apart -- one pair per word where a compare against both ends had two).
__device__ __forceinline__ void zero_tail(u32 (&m)[16], u32 r) {
    const int w = (int)(r >> 2);                         // the word the string ends in ...
    const u32 pm = ~(0xFFFFFFFFu << (8u * (r & 3u)));    // ... and its data bytes (none: r is a multiple of 4)
    u32 upto = 0xFFFFFFFFu;                              // all ones while k <= w
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const u32 below = (u32)((k - w) >> 31);          // all ones while k < w: the word is all data
        m[k] &= below | (upto & pm);
        upto = below;
    }
}

// lane-owned loads: the block starts at nx0.x, and a little-endian machine's dwords are the message words
__device__ __forceinline__ void block_words_lane(u32 (&m)[16], const u32x4& nx0, const u32x4& nx1, const u32x4& nx2,
                                                 const u32x4& nx3) {
    m[0] = nx0.x; m[1] = nx0.y; m[2] = nx0.z; m[3] = nx0.w;
    m[4] = nx1.x; m[5] = nx1.y; m[6] = nx1.z; m[7] = nx1.w;
    m[8] = nx2.x; m[9] = nx2.y; m[10] = nx2.z; m[11] = nx2.w;
    m[12] = nx3.x; m[13] = nx3.y; m[14] = nx3.z; m[15] = nx3.w;
}
// cooperative loads: the window is dword-aligned, `carry` is the dword in front of it, and `sel` (0x03020100 + 0x01010101
// x the string's misalignment) picks the four bytes of {hi, lo} that start at it: v_perm_b32, little-endian
__device__ __forceinline__ u32 le_word(u32 hi, u32 lo, u32 sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
__device__ __forceinline__ void block_words_coop(u32 (&m)[16], const u32x4& nx0, const u32x4& nx1, const u32x4& nx2,
                                                 const u32x4& nx3, u32& carry, u32 sel) {
    m[0] = le_word(nx0.x, carry, sel); m[1] = le_word(nx0.y, nx0.x, sel);
    m[2] = le_word(nx0.z, nx0.y, sel); m[3] = le_word(nx0.w, nx0.z, sel);
    m[4] = le_word(nx1.x, nx0.w, sel); m[5] = le_word(nx1.y, nx1.x, sel);
    m[6] = le_word(nx1.z, nx1.y, sel); m[7] = le_word(nx1.w, nx1.z, sel);
    m[8] = le_word(nx2.x, nx1.w, sel); m[9] = le_word(nx2.y, nx2.x, sel);
    m[10] = le_word(nx2.z, nx2.y, sel); m[11] = le_word(nx2.w, nx2.z, sel);
    m[12] = le_word(nx3.x, nx2.w, sel); m[13] = le_word(nx3.y, nx3.x, sel);
    m[14] = le_word(nx3.z, nx3.y, sel); m[15] = le_word(nx3.w, nx3.z, sel);
    carry = nx3.w;
}

}  // namespace

// The lane pipeline of sha256_items_kernel (sha256.hip, "Lane pipeline"): cur = the string being hashed with nx* = its NEXT
// 64 bytes, loaded one iteration ahead; next = the lane's next string, acquired kLook iterations before cur ends through
// (1) the wave-aggregated atomic dequeue, (1b) its resolution to a queue position, (2) the descriptor loads, (3) the load of
// its first 64 bytes -- each stage consumed one iteration after it was issued.  Reads run past a string's end exactly as far
// as that kernel's do (63 bytes, 67 with kCoop, 3 in front of a string that does not start on a dword; a block is fetched
// only when the string has a byte in it) and this kernel is launched on the same buffers, which carry that slack.
// kPass only names the instantiation so profiles tell the chunk pass from the root passes.
template <int kPass, bool kCoop>
__global__ __launch_bounds__(kShaWG)
void blake2s_items_kernel(const u8* __restrict__ base, const u64* __restrict__ off,
                          const u64* __restrict__ len, const u32* __restrict__ ids, u32 n_max,
                          const u64* __restrict__ n_ptr, u32* __restrict__ heads,
                          u32* __restrict__ roles, u32 long_shift, u8* __restrict__ out) {
    const u32 n = n_ptr ? (u32)*n_ptr : n_max;
    const int lane = threadIdx.x & 63;
    const int q0 = blockIdx.x % kShaQueues;
    // the wave's role on its SIMD: the first to arrive (the one the issue arbiter prefers, being the older) takes the long
    // strings [0, L), the others [L, n); whoever runs dry continues in the other range (sha256.hip)
    u32 role = 0;
    if (roles) {
        const u32 hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));        // HW_REG_HW_ID
        const u32 xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11)) & 7u; // HW_REG_XCC_ID
        const u32 key = (xcc << 10) | (((hw >> 8) & 0xFFu) << 2) | ((hw >> 4) & 3u);
        u32 r = 0;
        if (lane == 0) r = atomicAdd(roles + key, 1u);
        role = (u32)__builtin_amdgcn_readfirstlane((int)r);
        if (long_shift & 0x100u)  __builtin_amdgcn_s_setprio(0);
        else if (role == 0)       __builtin_amdgcn_s_setprio(3);
        else                      __builtin_amdgcn_s_setprio(1);
    }
    const u32 long_n = roles ? ((n >> (long_shift & 31u)) & ~(u32)(kShaQueues - 1)) : 0u;   // L, a multiple of the queue count
    const int my_set = role == 0 ? 0 : 1;
    const int qtry_end = (role == 0 || long_n) ? 2 * kShaQueues : kShaQueues;
    // current string
    const u8* ptr = nullptr;
    u64 rem = 0, total = 0;              // rem: bytes from the block in nx* to the end
    u32 slot = 0;
    u32 h[8];
    u32x4 nx0, nx1, nx2, nx3;
    // kCoop only:
    __shared__ __attribute__((aligned(16))) u32 xpose[kCoop ? kShaWG / 64 : 1][kCoop ? 64 * kXRow : 4];
    u32* xw = xpose[kCoop ? threadIdx.x >> 6 : 0];
    const int sub = lane & 3, qbase = lane & ~3;
    u32x4 g0 = {0, 0, 0, 0}, g1 = g0, g2 = g0, g3 = g0;
    bool loaded = false;
    u32 carry = 0, sel = 0x03020100u;
    u32 fc = 0;
    bool active = false;
    // next string
    enum : u32 { kNone = 0, kReq = 1, kPos = 2, kDesc = 3, kReady = 4, kDry = 5 };
    u32 nstate = kNone, npos = 0, nslot = 0, areq = 0, req_rank = 0;
    int req_q = 0, req_set = 0, req_leader = 0;
    u64 noff = 0, nlen = 0;
    u32x4 f0, f1, f2, f3;
    int qtry = (role == 0 && long_n == 0) ? kShaQueues : 0;

    for (;;) {
        // everything issued in the previous iteration has had a whole compression to land: consume it all here, before
        // this iteration issues anything new
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // incl. the hand-issued dequeue atomic
        asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3), "+v"(nx0), "+v"(nx1),
                          "+v"(nx2), "+v"(nx3));
        asm volatile("" : "+v"(noff), "+v"(nlen), "+v"(nslot), "+v"(areq));
        if constexpr (kCoop) asm volatile("" : "+v"(g0), "+v"(g1), "+v"(g2), "+v"(g3), "+v"(fc));
        if (kCoop && __ballot(loaded)) {
            // pieces -> owners: piece `sub` of owner qbase + m lies in g_m
            *(u32x4*)&xw[(qbase + 0) * kXRow + 4 * sub] = g0;
            *(u32x4*)&xw[(qbase + 1) * kXRow + 4 * sub] = g1;
            *(u32x4*)&xw[(qbase + 2) * kXRow + 4 * sub] = g2;
            *(u32x4*)&xw[(qbase + 3) * kXRow + 4 * sub] = g3;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (loaded) {
                nx0 = *(const u32x4*)&xw[lane * kXRow];
                nx1 = *(const u32x4*)&xw[lane * kXRow + 4];
                nx2 = *(const u32x4*)&xw[lane * kXRow + 8];
                nx3 = *(const u32x4*)&xw[lane * kXRow + 12];
                loaded = false;
            }
            __builtin_amdgcn_wave_barrier();               // the rows are rewritten next iteration
        }
        // ---- stage 1b: resolve last iteration's dequeue --------------------------------
        if (__ballot(nstate == kReq)) {
            const u32 first = __shfl(areq, req_leader);
            bool missed = false;
            if (nstate == kReq) {
                const u64 pos = (u64)(first + req_rank) * kShaQueues + (u32)req_q + (req_set ? long_n : 0u);
                if (pos < (req_set ? n : long_n)) { npos = (u32)pos; nstate = kPos; }
                else { nstate = kNone; missed = true; }
            }
            if (__ballot(missed)) ++qtry;              // a position past the end: that queue is dry
        }
        // ---- switch to the next string (its first block arrived an iteration ago) -------
        if (!active && nstate == kReady) {
            if constexpr (kCoop) {
                const u8* p = base + noff;
                const u32 mis = (u32)(size_t)p & 3u;
                ptr = p - mis + 4;                     // the aligned window behind the carried dword
                sel = 0x03020100u + mis * 0x01010101u;
                carry = fc;
            } else {
                ptr = base + noff;
            }
            total = rem = nlen;
            slot = nslot;
            nx0 = f0; nx1 = f1; nx2 = f2; nx3 = f3;
            blake2s_iv(h);
            active = true;
            nstate = kNone;
        }
        // ---- stage 3: descriptor known -> fetch the first block -----------------------
        if (nstate == kDesc) {
            const u8* p = base + noff;
            if (nlen) {
              if constexpr (kCoop) {
                // a string's FIRST block is fetched by its own lane; the dword in front through a laundered pointer
                // (sha256.hip: seen together, hipcc merges the five loads and waits for memory inside the iteration)
                const u8* q = p - ((size_t)p & 3u);
                typedef __attribute__((address_space(1))) const u32 glob_cu32;
                glob_cu32* qc = (glob_cu32*)q;
                asm volatile("" : "+v"(qc));
                fc = *qc;
                f0 = *(const u32x4_a4*)(q + 4);
                f1 = *(const u32x4_a4*)(q + 20);
                f2 = *(const u32x4_a4*)(q + 36);
                f3 = *(const u32x4_a4*)(q + 52);
              } else {
                f0 = *(const u32x4_unaligned*)(p);
                f1 = *(const u32x4_unaligned*)(p + 16);
                f2 = *(const u32x4_unaligned*)(p + 32);
                f3 = *(const u32x4_unaligned*)(p + 48);
              }
            }
            nstate = kReady;
        }
        // ---- stage 2: position known -> load its descriptor ---------------------------
        if (nstate == kPos) {
            noff = off[npos];
            nlen = len[npos];
            nslot = ids ? ids[npos] : npos;
            nstate = kDesc;
        }
        // ---- stage 1: reserve a position for lanes about to run dry -------------------
        {
            const bool want = nstate == kNone && (!active || rem < 64ull * kLook);
            const u64 mk = __ballot(want);
            u64 leader_mask = 0;                           // wave-uniform: the lane that performs the atomic
            if (mk) {
                if (qtry >= qtry_end) {
                    if (want) nstate = kDry;
                } else {
                    req_q = (q0 + qtry) % kShaQueues;
                    req_set = qtry < kShaQueues ? my_set : 1 - my_set;
                    req_leader = __ffsll((unsigned long long)mk) - 1;
                    leader_mask = 1ull << req_leader;
                    if (want) {
                        req_rank = (u32)__popcll(mk & ((1ull << lane) - 1ull));
                        nstate = kReq;
                    }
                }
            }
            // the atomic itself, in straight-line code and by hand (sha256.hip: behind a branch hipcc waits for its result);
            // EXEC is the leader lane alone, or empty: no request
            {
                u64 saved;
                const u32 cnt = (u32)__popcll(mk);
                const u32* head = heads + req_set * kShaQueues + req_q;
                asm volatile("s_mov_b64 %[sv], exec\n\t"
                             "s_mov_b64 exec, %[mk]\n\t"
                             "global_atomic_add %[ret], %[hd], %[val], off sc0\n\t"
                             "s_mov_b64 exec, %[sv]"
                             : [ret] "+v"(areq), [sv] "=&s"(saved)
                             : [mk] "s"(leader_mask), [val] "v"(cnt), [hd] "v"(head)
                             : "memory");
            }
        }
        if (!__ballot(active || nstate != kDry)) break;

        u32 m[16];
        bool last = false;
        bool want = false;                                 // kCoop: my string has another block to fetch
        if (active) {
            if constexpr (kCoop) block_words_coop(m, nx0, nx1, nx2, nx3, carry, sel);
            else                 block_words_lane(m, nx0, nx1, nx2, nx3);
            if (rem > 64) {                                // in flight during this block's ten rounds
                ptr += 64;
                rem -= 64;
                if constexpr (kCoop) {
                    want = true;
                } else {
                    nx0 = *(const u32x4_unaligned*)(ptr);
                    nx1 = *(const u32x4_unaligned*)(ptr + 16);
                    nx2 = *(const u32x4_unaligned*)(ptr + 32);
                    nx3 = *(const u32x4_unaligned*)(ptr + 48);
                }
            } else {                                       // the block that ends the string: 0..64 bytes of it
                if (rem < 64) zero_tail(m, (u32)rem);
                rem = 0;
                last = true;
            }
        }
        if (kCoop && __ballot(want)) {
            coop_fetch<false>(g0, g1, g2, g3, ptr, want, sub);
            loaded = want;
        }
        if (active) {
            blake2s_compress(h, m, total - rem, last);
            if (last) {
                u32x4* o = (u32x4*)(out + 32ull * slot);
                u32x4 d0, d1;
                d0.x = h[0]; d0.y = h[1]; d0.z = h[2]; d0.w = h[3];
                d1.x = h[4]; d1.y = h[5]; d1.z = h[6]; d1.w = h[7];
                o[0] = d0; o[1] = d1;
                active = false;
            }
        }
    }
}

// launch_sha256_items' contract (mi_common.h) and its geometry (sha_items_geometry, one function for both launchers), with
// ShaTune's values (what was tried on top of them).  Roots are one instantiation, everything else the chunk
// pass's.
void launch_blake2s_items(ShaPass pass, const u8* d_base, const u64* d_off, const u64* d_len,
                          const u32* d_order, u32 n, const u64* d_n, u32* d_heads, u32* d_roles, bool zero_heads,
                          u8* d_out, const ShaTune& tune, int n_cu, u64 footprint_bytes, hipStream_t s) {
    static thread_local int attr_dev = -1;
    ShaGeometry geo;
    u32 shift_flags;
    // up to FOUR workgroups per CU can be pinned: at 95 VGPRs five waves per SIMD fit; the lane-owned kernel has no static LDS
    if (!prepare_items_launch(geo, shift_flags, d_roles, pass, n, d_heads, zero_heads, tune, n_cu, footprint_bytes, 4, 0,
                              {(const void*)blake2s_items_kernel<kShaChunks, false>, (const void*)blake2s_items_kernel<kShaRoots, false>},
                              attr_dev, s))
        return;
#define MI_B2S_LAUNCH(P, C)                                                                              \
    hipLaunchKernelGGL((blake2s_items_kernel<P, C>), dim3(geo.grid), dim3(kShaWG), geo.lds_pad, s, d_base, d_off, \
                       d_len, d_order, n, d_n, d_heads, d_roles, shift_flags, d_out)
    if (pass == kShaRoots) MI_B2S_LAUNCH(kShaRoots, false);
    else if (geo.coop)     MI_B2S_LAUNCH(kShaChunks, true);
    else                   MI_B2S_LAUNCH(kShaChunks, false);
#undef MI_B2S_LAUNCH
}


// ---- the VALU roof of this file's compression (mi_blake2s_valu_roof), as sha256_roof_kernel is SHA-256's ----------
// ten rounds per lane and iteration over register data: no memory traffic, no queues, no tails
__global__ __launch_bounds__(kShaWG)
void blake2s_roof_kernel(u32* __restrict__ out, u32 blocks) {
    u32 h[8], m[16];
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = t * 0x9E3779B9u + (u32)i;
    u32 x = t * 0x85EBCA6Bu + 1u;
    for (u32 b = 0; b < blocks; ++b) {
#pragma unroll
        for (int i = 0; i < 16; ++i) { x = x * 1664525u + 1013904223u; m[i] = x ^ h[i & 7]; }
        blake2s_compress(h, m, 64ull * (b + 1), b + 1 == blocks);
    }
    u32 r = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) r ^= h[i];
    out[t] = r;
}

double measure_blake2s_valu_roof(int n_cu, int waves_per_simd, u32 blocks, u32* d_scratch, hipStream_t s,
                                 hipEvent_t e0, hipEvent_t e1) {
    return measure_valu_roof(blake2s_roof_kernel, n_cu, waves_per_simd, blocks, d_scratch, s, e0, e1);
}

}  // namespace mi

// The f32x6 arithmetic of gfx950, once: what csrc/sa_x6.hip (SA scales), csrc/chain_x6.hip (dense layer chains) and csrc/dense_x6.hip
// (dense layers with GroupNorm) share -- the opt-in arithmetic `mlp_dtype = "f32x6"`.
//
// Arithmetic contract (include/captra_hip.h "f32x6"): an fp32 number v is held as v = v0 + v1 + v2 EXACTLY, v0 = bf16(v),
// v1 = bf16(v - v0), v2 = bf16(v - v0 - v1) (round to nearest even; the two residuals are exact in fp32 and the third part has at most
// eight significant bits).  A layer is y = act(b + sum_k [w0 x0 + w0 x1 + w1 x0 + w1 x1 + w0 x2 + w2 x0]_k): the three dropped
// products (w1 x2, w2 x1, w2 x2) are <= 2^-24 |w x| each, the kept ones are exact in the matrix pipe, the sums are fp32 -- the
// result differs from the exact k-ascending fmaf chain (the metric's arithmetic, csrc/sa_pipe.hip) by fp32-roundoff-sized terms
// (tests/test_x6_gpu.py: <= 2e-6 of the layer's largest output), and NOT bit for bit.
#pragma once
#include "mfma_bf16.h"
#include <type_traits>

namespace {

typedef int x6_i32x4 __attribute__((ext_vector_type(4)));      // a buffer resource in scalar registers

constexpr int x6_cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int x6_pad4(int a) { return (a + 3) / 4 * 4; }

// ---- the split ---------------------------------------------------------------------------------------------------------------
// (a, b) -> the packed pairs of their three parts: 12 VALU per register pair.
// WHERE IT IS PINNED differs per kernel, on purpose.  Left alone, LLVM sinks the whole split (pure arithmetic) down to its first use --
// the next layer's first MFMA -- five tiles' worth of it end up in one block that no MFMA covers and their accumulators stay live
// until then (the 196-wide SA scale spills); the scheduling barriers around a group do not bind IR-level sinking, an asm statement
// that "modifies" the three results does.
//  * chain_x6.hip: x6_split2_pinned, the pin inside the split, for the input column and for every read-out unit alike;
//  * sa_x6.hip:    x6_split2, and sx_split_unit pins behind its call (the same place; it is that kernel's only split);
//  * dense_x6.hip: x6_split2, no pin: the parts go straight to LDS, and a store is not sunk; its masked sched_barriers place them.
static __device__ __forceinline__ void x6_split2(float a, float b, unsigned &p0, unsigned &p1, unsigned &p2) {
    p0 = bf_pack(a, b);
    const float ra = a - bf_lo(p0), rb = b - bf_hi(p0);
    p1 = bf_pack(ra, rb);
    p2 = bf_pack(ra - bf_lo(p1), rb - bf_hi(p1));
}
static __device__ __forceinline__ void x6_split2_pinned(float a, float b, unsigned &p0, unsigned &p1, unsigned &p2) {
    x6_split2(a, b, p0, p1, p2);
    asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2));
}
// The same split of one weight on scalars, as the image builders write it: the bf16 bits of part 0 / 1 / 2 of v
static __device__ __forceinline__ unsigned short x6_part_bits(float v, int part) {
    const __bf16 h0 = (__bf16)v;
    const float r1 = v - (float)h0;
    const __bf16 h1 = (__bf16)r1;
    const __bf16 h2 = (__bf16)(r1 - (float)h1);
    const __bf16 h = part == 0 ? h0 : (part == 1 ? h1 : h2);
    return __builtin_bit_cast(unsigned short, h);
}

// ---- the six products --------------------------------------------------------------------------------------------------------
// One k-step as TWO accumulator chains issued alternately -- `lo` takes the three small products (2^-16 of the leading one), `hi` the
// three large ones; a tile's result is hi + lo.  Back-to-back MFMAs on ONE accumulator run at the issue rate only while nothing sits
// between them: every ds_read / VALU the scheduler puts into such a chain costs ~43 cycles (MI355X_MICROARCH.md), and a k-step carries
// three fragment reads -- one chain ran the matrix pipe at 0.62-0.68; between MFMAs on different accumulators a filler costs ~6.
// The issue order below is part of the schedule.  FLIP: activations are the A operand (rows = positions)
template <bool FLIP>
static __device__ __forceinline__ void x6_group(f32x16 &hi, f32x16 &lo, const u32x4 (&w)[3], const u32x4 &x0, const u32x4 &x1, const u32x4 &x2) {
    if constexpr (FLIP) {
        lo = bf_mfma(x0, w[2], lo); hi = bf_mfma(x0, w[1], hi); lo = bf_mfma(x2, w[0], lo);
        hi = bf_mfma(x1, w[0], hi); lo = bf_mfma(x1, w[1], lo); hi = bf_mfma(x0, w[0], hi);
    } else {
        lo = bf_mfma(w[2], x0, lo); hi = bf_mfma(w[1], x0, hi); lo = bf_mfma(w[0], x2, lo);
        hi = bf_mfma(w[0], x1, hi); lo = bf_mfma(w[1], x1, lo); hi = bf_mfma(w[0], x0, hi);
    }
}

// compile-time loop: f(std::integral_constant<int, I>) for I in [0, N) -- the body sees I as a constant expression (the
// scheduling-group builtins want integer constants)
template <int I, int N, typename F>
static __device__ __forceinline__ void x6_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        x6_static_for<I + 1, N>(f);
    }
}
// the group of the NEXT tile's k-steps behind whose MFMAs unit u (0..7) of a deferred split epilogue is issued: none in group 0
// (the tile's last MFMA is still executing), spread over groups 1 .. KST - 1
constexpr int x6_unit_group(int u, int kst) { return kst > 1 ? 1 + u * (kst - 1) / 8 : 0; }

// ---- weights on their way into LDS ---------------------------------------------------------------------------------------------
// s_waitcnt with only the vector-memory counter set (gfx9 encoding: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt[5:4] << 14)
#define X6_WAIT_VM(N) __builtin_amdgcn_s_waitcnt(((N) & 15) | (((N) >> 4) << 14) | 0x0F70)

// One LDS-DMA piece: 64 lanes x 16 bytes from rsrc at byte soff + voff16 (voff16 = lane x 16) to the LDS byte address lds_dst
// (wave-uniform; the hardware adds lane x 16).
// It is an asm statement: hipcc (ROCm 7.2) orders every LDS read it can see behind ALL LDS-DMA in flight (s_waitcnt vmcnt(0) in front
// of the first ds_read after an issue -- the bias reads of the next tile: a prefetch would wait for itself), and it keeps a 64-bit
// per-lane address per piece of the global form and spills them.  Buffer form: one VGPR of lane offsets, the piece's place in the image
// as a scalar offset; m0 = the piece's LDS address, one s_nop between its write and the load that reads it.  The compiler's own vmcnt
// waits stay safe: loads return in order, pieces it does not know of only make it wait longer.
static __device__ __forceinline__ void x6_lds_dma(unsigned lds_dst, unsigned voff16, x6_i32x4 rsrc, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds"
                 :: "s"(lds_dst), "v"(voff16), "s"(rsrc), "s"(soff) : "memory");
}

// The weight ring of sa_x6.hip (RING) and chain_x6.hip: three LDS slots, chunk c (one row tile) in slot c % 3, filled by the four
// waves of the workgroup together -- wave w issues the fragments 4 i + w of a chunk of `frags` (a multiple of four).  lds_slot: the
// slot's LDS byte address, img_off: the chunk's byte offset in the image.
static __device__ __forceinline__ void x6_ring_issue(unsigned lds_slot, unsigned voff16, x6_i32x4 rsrc, unsigned img_off, int wave, int frags) {
    const unsigned dst = lds_slot + wave * 1024, soff = img_off + wave * 1024;
#pragma unroll
    for (int i = 0; i < frags / 4; ++i) x6_lds_dma(dst + i * 4096, voff16, rsrc, soff + i * 4096);
}

// ---- the hand-over weight image --------------------------------------------------------------------------------------------------
// The fragment block of one layer (cin -> cout) as sa_x6.hip (layers 2, 3) and chain_x6.hip (every layer) read it: row tile t is one
// CHUNK of x6_pad4(3 kst) fragments of 1 KiB, k-step major (fragment 3 kk + part, byte kk * 3072 + part * 1024 + lane * 16 of the
// chunk; padded so that the four waves of a workgroup issue the same number of LDS-DMA pieces).  Lane l of a fragment = row
// 32 t + (l & 31), k-slots 8 (l >> 5) .. + 7 of k-step kk; slot s holds channel 16 kk + perm(s) (the in-register hand-over order) or
// 16 kk + s (natural: a layer whose operand is loaded in channel order).  wt: the layer's packed fp32 W'^T (row-major part, element
// [k * ldw + cout]).  Returns the bf16 bits of element e (0 .. nt * chunk * 512) of the block.
static __device__ __forceinline__ unsigned short x6_frag_bits(long long e, int cin, int cout, int ldw, bool natural, const float *wt) {
    const int kst = x6_cdiv(cin, 16), ch = x6_pad4(kst * 3);
    const int f = (int)(e >> 9), lane = (int)(e >> 3) & 63, el = (int)e & 7;
    const int slot = 8 * (lane >> 5) + el;
    const int t = f / ch, r = f % ch, kk = r / 3, part = r % 3;
    const int row = 32 * t + (lane & 31), k = 16 * kk + (natural ? slot : bf_perm(slot));
    float v = 0.f;
    if (kk < kst && row < cout && k < cin) v = wt[(size_t)k * ldw + row];
    return x6_part_bits(v, part);
}

}  // namespace

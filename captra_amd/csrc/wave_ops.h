// The cross-lane primitives of wave64 on gfx950, defined once: DPP moves, the reductions over a row of 16 lanes and over the wave
// built on them, the xor-butterfly reductions over __shfl_xor, and the workgroup sum.  (v_permlane32_swap, ds_swizzle and the
// arg-max-with-index shuffles stay with the kernels that use them.)
#pragma once
#include "common.h"

// ---- DPP moves: lane l reads `src` of the lane CTRL names; ROW_MASK / BANK_MASK pick the rows of 16 / banks of 4 lanes that take part.
// dpp_keep: a lane without a valid source, or outside the masks, gets `old` (the one-argument form: its own value).  Always legal.
// dpp_zero: such a lane gets 0 (bound_ctrl) -- the form the compiler folds into the operation (v_max_u32_dpp, v_add_f32_dpp,
// v_max_i32_dpp: one instruction instead of a move and the operation).  Legal ONLY where 0 is the operation's identity: an unsigned
// max, a sum, a max with a value that is already >= 0 -- or where every lane has a source (quad_perm, row_ror within full masks).
// That is why the unsigned MINIMUM has no zero form of its own: wave_min_u32 keeps its own value, and the pruned sampler's
// wave_min_u32_fold is ~max(~v).
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ int dpp_keep(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, BANK_MASK, false);
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ unsigned dpp_keep(unsigned old, unsigned src) {
    return (unsigned)dpp_keep<CTRL, ROW_MASK, BANK_MASK>((int)old, (int)src);
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ float dpp_keep(float old, float src) {
    return __int_as_float(dpp_keep<CTRL, ROW_MASK, BANK_MASK>(__float_as_int(old), __float_as_int(src)));
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF, class T>
static __device__ __forceinline__ T dpp_keep(T v) { return dpp_keep<CTRL, ROW_MASK, BANK_MASK>(v, v); }

template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ int dpp_zero(int src) {
    return __builtin_amdgcn_update_dpp(0, src, CTRL, ROW_MASK, BANK_MASK, true);
}
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ unsigned dpp_zero(unsigned src) { return (unsigned)dpp_zero<CTRL, ROW_MASK, BANK_MASK>((int)src); }
template <int CTRL, int ROW_MASK = 0xF, int BANK_MASK = 0xF>
static __device__ __forceinline__ float dpp_zero(float src) {
    return __int_as_float(dpp_zero<CTRL, ROW_MASK, BANK_MASK>(__float_as_int(src)));
}

// ---- reductions over a row of 16 lanes (every lane of the row holds the row's result) and over the wave.  FOLD picks the move.
template <bool FOLD, int CTRL, int ROW_MASK = 0xF, class T>
static __device__ __forceinline__ T dpp_partner(T v) {
    if constexpr (FOLD) return dpp_zero<CTRL, ROW_MASK>(v);
    else return dpp_keep<CTRL, ROW_MASK>(v);
}
template <bool FOLD, class T, class Op>
static __device__ __forceinline__ T row16_reduce(T v, Op op) {
    v = op(v, dpp_partner<FOLD, 0xB1>(v));    // quad_perm [1,0,3,2]
    v = op(v, dpp_partner<FOLD, 0x4E>(v));    // quad_perm [2,3,0,1]
    v = op(v, dpp_partner<FOLD, 0x141>(v));   // row_half_mirror
    v = op(v, dpp_partner<FOLD, 0x140>(v));   // row_mirror
    return v;
}
// ... over the wave: the result is lane 63's, returned wave-uniform (an SGPR)
template <bool FOLD, class Op>
static __device__ __forceinline__ unsigned wave64_reduce_u32(unsigned v, Op op) {
    v = row16_reduce<FOLD>(v, op);
    v = op(v, dpp_partner<FOLD, 0x142, 0xA>(v));   // row_bcast15 -> rows 1, 3
    v = op(v, dpp_partner<FOLD, 0x143, 0xC>(v));   // row_bcast31 -> rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
struct UMaxOp { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return max(a, b); } };
struct UMinOp { __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return min(a, b); } };

static __device__ __forceinline__ unsigned row_max_u32(unsigned v) { return row16_reduce<false>(v, UMaxOp()); }
static __device__ __forceinline__ unsigned row_min_u32(unsigned v) { return row16_reduce<false>(v, UMinOp()); }
static __device__ __forceinline__ unsigned wave_max_u32(unsigned v) { return wave64_reduce_u32<false>(v, UMaxOp()); }
static __device__ __forceinline__ unsigned wave_min_u32(unsigned v) { return wave64_reduce_u32<false>(v, UMinOp()); }
static __device__ __forceinline__ unsigned row_max_u32_fold(unsigned v) { return row16_reduce<true>(v, UMaxOp()); }
static __device__ __forceinline__ unsigned wave_max_u32_fold(unsigned v) { return wave64_reduce_u32<true>(v, UMaxOp()); }
static __device__ __forceinline__ unsigned wave_min_u32_fold(unsigned v) { return ~wave_max_u32_fold(~v); }
static __device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
// the max pools' row step, on the non-negative bit patterns of relu_pool_bits (common.h: a NaN above +Inf; fmaxf would drop it)
static __device__ __forceinline__ int row16_maxi(int v) { return row16_reduce<false>(v, [](int a, int b) { return imax(a, b); }); }
// sum over each half-wave (32 lanes): valid in lanes 16..31 (lower half) and 48..63 (upper half)
static __device__ __forceinline__ float half_wave_sum(float v) {
    v = row16_reduce<true>(v, [](float a, float b) { return a + b; });
    return v + dpp_zero<0x142, 0xA>(v);            // row_bcast15: rows 1 and 3 add rows 0 and 2
}

// max(own, oth of the partner lane) for a permutation in which EVERY lane has a source (quad_perm, row_ror): one v_max_i32_dpp
template <int CTRL>
static __device__ __forceinline__ int imax_dpp(int own, int oth) {
    const int o = dpp_zero<CTRL>(oth);
    return o > own ? o : own;
}

// ---- xor butterflies over __shfl_xor: every lane holds the result.  `from` = the first xor distance: 32 reduces the wave, 16 each
// half-wave of 32 lanes.  The butterfly is defined once, as a STATEMENT: WAVE_BUTTERFLY(v, from, op) leaves op over the lanes in v.
// The functions below wrap it; a kernel that reduces the registers of an unrolled loop in place uses the statement, because a
// function's loop is unrolled before it is inlined, the lane arithmetic of __shfl_xor is then hoisted out of the caller's register
// loop, and the hot kernels would get another schedule.
#define WAVE_BUTTERFLY(v, from, op) \
    _Pragma("unroll") for (int wb_off = (from); wb_off >= 1; wb_off >>= 1) v = op(v, __shfl_xor(v, wb_off, 64))
// ... and two values step by step in one loop (the order gn_finalize and the ball query's bounding box issue their shuffles in)
#define WAVE_BUTTERFLY2(v0, op0, v1, op1, from)                                       \
    _Pragma("unroll") for (int wb_off = (from); wb_off >= 1; wb_off >>= 1) {          \
        v0 = op0(v0, __shfl_xor(v0, wb_off, 64));                                     \
        v1 = op1(v1, __shfl_xor(v1, wb_off, 64));                                     \
    }
template <class T>
static __device__ __forceinline__ T wave_add(T a, T b) { return a + b; }

static __device__ __forceinline__ float wave_minf(float v) {
    WAVE_BUTTERFLY(v, 32, fminf);
    return v;
}
static __device__ __forceinline__ float wave_maxf(float v) {
    WAVE_BUTTERFLY(v, 32, fmaxf);
    return v;
}

// ---- the workgroup sum of NV values over NW waves: per-wave butterfly, barrier, lane 0 of every wave stores smem[i * NW + wave],
// barrier, combine.  The order of the combine is part of the bit contract of the kernels that use it:
//   WG_SUM_PAIRS  (w0 + w1) + (w2 + w3), NW = 4: part_fit_st / procrustes_rot3 (pose_fit.hip), group_norm_relu (track_ops.hip)
//                 and rp_pool_compose (rot_pool.h), which calls the two halves itself: under rot_consensus.hip's sixteen waves
//                 only the first four store, and thread 0 alone combines;
//   WG_SUM_SERIAL ((0 + w0) + w1) + ... upward, NW = 16: the refit sums of rs_fit (pose_ransac.h) and the guard's residual sum.
enum WgSumOrder { WG_SUM_PAIRS, WG_SUM_SERIAL };

// v -> the wave's sums, lane 0's into smem where `stores` (uniform over the wave); ends with a barrier
template <int NW, int NV, class T>
static __device__ __forceinline__ void wg_sum_publish(T (&v)[NV], T *smem /* [NV][NW] */, bool stores = true) {
#pragma unroll
    for (int i = 0; i < NV; ++i) WAVE_BUTTERFLY(v[i], 32, wave_add);
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && stores)
#pragma unroll
        for (int i = 0; i < NV; ++i) smem[i * NW + (threadIdx.x >> 6)] = v[i];
    __syncthreads();
}
template <WgSumOrder ORDER, int NW, int NV, class T>
static __device__ __forceinline__ void wg_sum_combine(T (&v)[NV], const T *smem) {
    static_assert(ORDER == WG_SUM_SERIAL || NW == 4, "the pairwise order adds four waves");
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if constexpr (ORDER == WG_SUM_PAIRS) {
            v[i] = (smem[i * 4 + 0] + smem[i * 4 + 1]) + (smem[i * 4 + 2] + smem[i * 4 + 3]);
        } else {
            T x = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) x += smem[i * NW + w];
            v[i] = x;
        }
    }
}
// every thread of the workgroup calls it and gets the sums
template <WgSumOrder ORDER, int NW, int NV, class T>
static __device__ __forceinline__ void wg_sum(T (&v)[NV], T *smem /* [NV][NW] */) {
    wg_sum_publish<NW>(v, smem);
    wg_sum_combine<ORDER, NW>(v, smem);
}
template <WgSumOrder ORDER, int NW, class T>
static __device__ __forceinline__ T wg_sum(T v, T *smem /* [NW] */) {
    T a[1] = {v};
    wg_sum<ORDER, NW>(a, smem);
    return a[0];
}

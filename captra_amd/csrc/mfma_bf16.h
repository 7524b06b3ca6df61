// The bf16 pair primitives of gfx950, shared by every kernel that feeds v_mfma_f32_32x32x16_bf16 with operands it packs itself: the
// bf16 SA scales (csrc/sa_bf16.hip), the bf16 dense kernels (csrc/bf16_dense.h and its users) and the f32x6 kernels (csrc/x6.h).
// (csrc/bf16_mlp.hip keeps its own pack_bf16: two scalar casts, other instructions, on purpose.)
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// (lo, hi) -> a packed bf16 pair, RNE: one v_cvt_pk_bf16_f32 (the vector fptrunc; two scalar casts compile to two conversions and a
// v_perm_b32)
static __device__ __forceinline__ unsigned bf_pack(float lo, float hi) {
    const f32x2 f = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
// the halves of a packed pair as fp32 (exact)
static __device__ __forceinline__ float bf_lo(unsigned p) { return __uint_as_float(p << 16); }
static __device__ __forceinline__ float bf_hi(unsigned p) { return __uint_as_float(p & 0xffff0000u); }
// ReLU on a packed pair (a negative bf16 is a negative int16: one v_pk_max_i16)
static __device__ __forceinline__ unsigned bf_relu2(unsigned v) {
    const s16x2 z = {0, 0};
    return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, v), z));
}
static __device__ __forceinline__ f32x16 bf_mfma(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// ZERO-SWAP HAND-OVER (csrc/sa_bf16.hip): an accumulator tile is the next layer's operand as it stands when slot s of that layer's
// 16-wide k-step holds channel perm(s) = {0,1,2,3,8,9,10,11,4,5,6,7,12,13,14,15}[s]
__host__ __device__ constexpr int bf_perm(int s) { return (s & 3) | ((s & 4) << 1) | ((s & 8) >> 1); }

}  // namespace

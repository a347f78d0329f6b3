// What the f16x3 / bf16x6 translation units share: gemm.hip (the conv / linear / bank /
// highway GEMM family), highway_stack.hip and split_weights.hip.
#pragma once
#include "common.h"

namespace ftmi_gemm __attribute__((visibility("hidden"))) {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// matrix-fragment type and MFMA of the pre-split kernels: bf16 pieces (x6) or f16 (h3)
template <bool H3>
struct Frag {
  typedef bf16x8 T;
};
template <>
struct Frag<true> {
  typedef f16x8 T;
};
__device__ __forceinline__ f32x4 mma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

constexpr float H3_SCALE = 2048.f;  // 2^11: the tail scale of the f16 split

// a = a_h + 2^-11 a_t  (f16 head, scaled f16 tail)
__device__ __forceinline__ void split2h(f32x4 v, f16x4 &h, f16x4 &t) {
  h = __builtin_convertvector(v, f16x4);
  t = __builtin_convertvector((v - __builtin_convertvector(h, f32x4)) * H3_SCALE, f16x4);
}

// highway output g relu(x1) + (1 - g) x with one fixed rounding sequence in every kernel
// (no compiler-chosen contraction: the fused stack is bit-identical to the per-layer path)
__device__ __forceinline__ float highway_mix(float g, float x1, float x) {
#pragma clang fp contract(off)
  return fmaf(g, fmaxf(x1, 0.f), (1.f - g) * x);
}

constexpr int X6_BK = 32;

__device__ __forceinline__ f32x4 fmax4(f32x4 a, f32x4 b) {
  f32x4 r;
  r.x = fmaxf(a.x, b.x);
  r.y = fmaxf(a.y, b.y);
  r.z = fmaxf(a.z, b.z);
  r.w = fmaxf(a.w, b.w);
  return r;
}

// bytes of one weight's pre-split block: bf16 pieces (mma = 1) or f16 planes + colscale
inline int64_t split_block_bytes(int64_t N, int64_t K, int mma) {
  const int64_t planes = 3 * N * ((K + X6_BK - 1) / X6_BK * X6_BK) * 2;
  return mma == 2 ? planes + (4 * N + 15) / 16 * 16 : planes;
}

}  // namespace ftmi_gemm

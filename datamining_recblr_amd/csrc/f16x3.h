// f16x3.h — the device primitives of the f16 two-part split ("f16x3": three
// MFMA products per k-step; the scheme and its error bound are described at
// the top of gemm_half.hip).  An operand is scaled by an exact power of two,
// split into a hi and a lo fp16 part, the three significant products are
// accumulated in fp32 and the result is un-scaled with v_ldexp.  Device code
// only; the weight image's layout and scale are in common.h.
#pragma once

#include "common.h"
#include "lane_lds.h"

namespace rb {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// frexp exponent of a maximum (0 for an all-zero row or column)
__device__ __forceinline__ int exp_of(float m) {
  return m > 0.0f ? __builtin_amdgcn_frexp_expf(m) : 0;
}

// 2 fp32 (already scaled) -> hi, lo fp16 pairs (v_cvt_pk_f16_f32, RNE; the
// residual is exact in fp32)
__device__ __forceinline__ void split2h(f32x2 x, f16x2& h0, f16x2& h1) {
  h0 = __builtin_convertvector(x, f16x2);
  const f32x2 r = x - __builtin_convertvector(h0, f32x2);
  h1 = __builtin_convertvector(r, f16x2);
}

// 8 fp32 (p, q) times sc -> one MFMA fragment of each part
__device__ __forceinline__ void split8(f32x4 p, f32x4 q, float sc, f16x8& a0, f16x8& a1) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const f32x2 v = (t < 2 ? f32x2{p[2 * t], p[2 * t + 1]} : f32x2{q[2 * t - 4], q[2 * t - 3]}) * sc;
    f16x2 h0, h1;
    split2h(v, h0, h1);
    a0[2 * t] = h0[0]; a0[2 * t + 1] = h0[1];
    a1[2 * t] = h1[0]; a1[2 * t + 1] = h1[1];
  }
}

__device__ __forceinline__ f32x16 mfma_h(f16x8 a, f16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// The three products of one k-step, the small partial products first.  The
// order is part of the result's bits.  32x32x16: a1.b0, a0.b1, a0.b0.
__device__ __forceinline__ f32x16 mfma3_h(f16x8 a0, f16x8 a1, f16x8 b0, f16x8 b1, f32x16 c) {
  c = mfma_h(a1, b0, c);
  c = mfma_h(a0, b1, c);
  return mfma_h(a0, b0, c);
}
// 16x16x32 (gemm_ws.hip: the weight slice is the first operand a, so in
// terms of activation x and weight w this is mfma3_h's x1.w0, x0.w1, x0.w0):
// a0.b1, a1.b0, a0.b0.
__device__ __forceinline__ f32x4 mfma3_16(f16x8 a0, f16x8 a1, f16x8 b0, f16x8 b1, f32x4 c) {
  c = mfma16(a0, b1, c);
  c = mfma16(a1, b0, c);
  return mfma16(a0, b0, c);
}

// max(|a|, |b|, |c|) in one instruction (no NaN canonicalisation: a NaN input
// propagates to the output through the MFMA anyway)
__device__ __forceinline__ float max3abs(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float max4abs(f32x4 x) {
  float m, r;
  asm("v_max3_f32 %0, |%1|, |%2|, |%3|" : "=v"(m) : "v"(x[0]), "v"(x[1]), "v"(x[2]));
  asm("v_max_f32 %0, %1, |%2|" : "=v"(r) : "v"(m), "v"(x[3]));
  return r;
}
__device__ __forceinline__ float max8abs(f32x4 x, f32x4 y) {
  float m = max3abs(x[0], x[1], x[2]);
  m = max3abs(m, x[3], y[0]);
  m = max3abs(m, y[1], y[2]);
  float r;
  asm("v_max_f32 %0, %1, |%2|" : "=v"(r) : "v"(m), "v"(y[3]));
  return r;
}

}  // namespace rb

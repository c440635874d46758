// row_group.h — the scoring core of the gathered-row kernels (pair_loss.hip,
// candidates.hip): a 16-lane group computes one (h row, table row) dot
// product from 16-B loads, reduced inside the group.  A score is a pure
// function of the two rows' d floats, so every kernel built on dot_rows gives
// a pair the same bits.
#pragma once

#include "common.h"

namespace rb {

constexpr int kGroup = 16;              // lanes per row
constexpr int kGroups = 256 / kGroup;   // groups per 256-thread workgroup

// Both run over the whole wave: a caller keeps its code uniform (ids clamped
// for the loads, results masked) so that every lane takes part in the shuffles.
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = kGroup / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kGroup);
  return v;
}

__device__ __forceinline__ int group_or(int v) {
#pragma unroll
  for (int o = kGroup / 2; o > 0; o >>= 1) v |= __shfl_xor(v, o, kGroup);
  return v;
}

// lane l's float4s of row p [d]: columns 4 (l + 16 k), zeros past d
template <int NV4>
__device__ __forceinline__ void load_row(float4 (&o)[NV4], const float* p, int l, int d) {
#pragma unroll
  for (int k = 0; k < NV4; ++k) {
    const int col = 4 * (l + kGroup * k);
    o[k] = col < d ? *reinterpret_cast<const float4*>(p + col) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// the only place a score is computed
template <int NV4>
__device__ __forceinline__ float dot_rows(const float4 (&a)[NV4], const float4 (&b)[NV4]) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < NV4; ++k)
    s += (a[k].x * b[k].x + a[k].y * b[k].y) + (a[k].z * b[k].z + a[k].w * b[k].w);
  return group_sum(s);
}

// float4 loads per lane of a 16-lane group: d <= 64 * NV4
inline int row_vecs(int64_t d) { return d <= 64 ? 1 : d <= 128 ? 2 : d <= 256 ? 4 : 8; }

// f(std::integral_constant<int, NV4>{}) for d's NV4
template <class F>
void dispatch_row_vecs(int64_t d, F&& f) {
  dispatch_int<1, 2, 4, 8>(row_vecs(d), f);
}

}  // namespace rb

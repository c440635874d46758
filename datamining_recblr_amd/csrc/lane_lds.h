// lane_lds.h — the register vector types and the type-agnostic lane, LDS and
// wait wrappers of the MFMA GEMMs.  A header of its own (not a section of
// f16x3.h) so that gemm_bf16.hip includes no fp16 code.  Device code only.
#pragma once

#include "common.h"

namespace rb {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// ---- LDS accesses the compiler does not see (the caller places the
// s_waitcnt lgkmcnt and ties it to the destination registers); OFF: the
// instruction's immediate byte offset
template <typename T>
__device__ __forceinline__ T lds_read16(uint32_t addr) {
  T r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <int OFF, typename T>
__device__ __forceinline__ T lds_read16o(uint32_t addr) {
  T r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}
__device__ __forceinline__ int lds_read_i32(uint32_t addr) {
  int r;
  asm volatile("ds_read_b32 %0, %1" : "=v"(r) : "v"(addr));
  return r;
}
template <typename T>
__device__ __forceinline__ void lds_write16(uint32_t addr, T v) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
template <int OFF, typename T>
__device__ __forceinline__ void lds_write8(uint32_t addr, T v) {
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

// at most N vector-memory operations of this wave still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// quad_perm DPP moves (lane k of each quad reads lane k ^ 1 / k ^ 2)
__device__ __forceinline__ float dpp_xor1(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ float dpp_xor2(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, false));
}

// 4 x 4 transpose inside each lane quad: on entry lane k of a quad holds
// column k (v[r] = row r), on exit row k (v[c] = column c).  Two butterfly
// stages (lane distance 2, then 1), each a select + DPP move + select.
__device__ __forceinline__ void quad_transpose(float (&v)[4], int lane) {
  const bool b1 = (lane & 2) != 0, b0 = (lane & 1) != 0;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const float y = dpp_xor2(b1 ? v[r] : v[r + 2]);
    if (b1) v[r] = y; else v[r + 2] = y;
  }
#pragma unroll
  for (int r = 0; r < 4; r += 2) {
    const float y = dpp_xor1(b0 ? v[r] : v[r + 1]);
    if (b0) v[r] = y; else v[r + 1] = y;
  }
}

}  // namespace rb

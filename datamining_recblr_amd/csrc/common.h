// common.h — shared device helpers for the RecBLR gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/recblr_hip.h"
#include "../../include/recblr_dense.h"
#include "../../include/recblr_pairs.h"
#include "../../include/recblr_candidates.h"
#include "../../include/recblr_filters.h"
#include "../../include/recblr_groups.h"
#include "../../include/recblr_priors.h"

namespace rb {

constexpr int kWave = 64;

// ---- error reporting (host) -------------------------------------------------
int fail(const char* msg);
int launch_status(const char* what);
// compute units of the current device (cached per device)
int num_cus();

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- run-time values as template arguments (host) ----------------------------
// f(std::true_type{}) or f(std::false_type{})
template <class F>
auto dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}
// f(std::integral_constant<int, V>{}) for the V among Vs that equals v;
// false when none does
template <int... Vs, class F>
bool dispatch_int(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- scalar math, following torch's definitions ------------------------------
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
// torch.nn.functional.softplus(beta=1, threshold=20)
__device__ __forceinline__ float softplus_f(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float dsoftplus_f(float x) { return x > 20.0f ? 1.0f : sigm(x); }
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + expf(-x)); }
// d/dx silu(x) = s (1 + x (1 - s)), s = sigmoid(x)
__device__ __forceinline__ float dsilu_f(float x) {
  const float s = sigm(x);
  return s * (1.0f + x * (1.0f - s));
}

// ---- hardware transcendentals (v_exp_f32 / v_rcp_f32 / v_sqrt_f32, ~1 ulp) ----
// The libm forms above expand to ~10-15 instructions each (range reduction,
// IEEE division); in the [B, L, H] kernels they made the VALU co-bound with
// HBM.  The native forms keep every quantity within a few ulp, which stays
// far inside the 1e-4 parity budget: the one cancellation-prone value,
// 1 - alpha^2 with alpha -> 0.999, depends on alpha's absolute error (~ulp(1))
// exactly as it does with expf.
constexpr float kLog2e = 1.4426950408889634f;
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * kLog2e); }
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fsigm(float x) { return frcp(1.0f + fexp(-x)); }
__device__ __forceinline__ float fsilu(float x) { return x * fsigm(x); }
__device__ __forceinline__ float fdsilu(float x) {
  const float s = fsigm(x);
  return s * (1.0f + x * (1.0f - s));
}

// ---- VEC-wide loads/stores (VEC = 4 -> one 16-B access per lane) -------------
// Every [B, L, H] stream is read or written once per kernel, so the accesses
// carry the nontemporal hint (global_load/store ... nt): on this chip a plain
// 1R+1W float4 copy runs at 0.76 of 8 TB/s with default-policy accesses and
// 0.83 with nt ones (tools/copyprobe2.hip, profiles/r01_copyprobe2.log).
typedef float rb_f32x4 __attribute__((ext_vector_type(4)));
typedef float rb_f32x2v __attribute__((ext_vector_type(2)));
typedef uint32_t rb_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t rb_u32x2 __attribute__((ext_vector_type(2)));

template <bool NT, typename T>
__device__ __forceinline__ T ld_pol(const T* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void st_pol(T v, T* p) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
constexpr bool kNT = true;

// ldv / stv: once-touched activation streams (nt); ldc / stc: default policy,
// for small operands many workgroups re-read (parameters, carries) and for
// inputs that neighbouring tiles re-read (the conv's halo rows).
template <bool NT, int V>
__device__ __forceinline__ void ld_f32(float (&o)[V], const float* p) {
  if constexpr (V == 4) {
    const rb_f32x4 t = ld_pol<NT>(reinterpret_cast<const rb_f32x4*>(p));
    o[0] = t[0]; o[1] = t[1]; o[2] = t[2]; o[3] = t[3];
  } else if constexpr (V == 2) {
    const rb_f32x2v t = ld_pol<NT>(reinterpret_cast<const rb_f32x2v*>(p));
    o[0] = t[0]; o[1] = t[1];
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = ld_pol<NT>(p + v);
  }
}

template <bool NT, int V>
__device__ __forceinline__ void st_f32(float* p, const float (&o)[V]) {
  if constexpr (V == 4) {
    st_pol<NT>(rb_f32x4{o[0], o[1], o[2], o[3]}, reinterpret_cast<rb_f32x4*>(p));
  } else if constexpr (V == 2) {
    st_pol<NT>(rb_f32x2v{o[0], o[1]}, reinterpret_cast<rb_f32x2v*>(p));
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) st_pol<NT>(o[v], p + v);
  }
}

template <int V>
__device__ __forceinline__ void ldv(float (&o)[V], const float* p) { ld_f32<kNT>(o, p); }
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&o)[V]) { st_f32<kNT>(p, o); }
template <int V>
__device__ __forceinline__ void ldc(float (&o)[V], const float* p) { ld_f32<false>(o, p); }
template <int V>
__device__ __forceinline__ void stc(float* p, const float (&o)[V]) { st_f32<false>(p, o); }

// ---- bf16 storage (fp32 arithmetic): VEC bf16 per lane, RNE on store ---------
typedef __bf16 bf16_t;
typedef __bf16 rb_bf16x2 __attribute__((ext_vector_type(2)));
typedef float rb_f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void unpack2(uint32_t u, float& a, float& b) {
  a = __uint_as_float(u << 16);
  b = __uint_as_float(u & 0xffff0000u);
}
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(rb_f32x2{a, b}, rb_bf16x2));
}

template <bool NT, int V>
__device__ __forceinline__ void ld_b16(float (&o)[V], const bf16_t* p) {
  if constexpr (V == 8) {
    const rb_u32x4 t = ld_pol<NT>(reinterpret_cast<const rb_u32x4*>(p));
    unpack2(t[0], o[0], o[1]); unpack2(t[1], o[2], o[3]);
    unpack2(t[2], o[4], o[5]); unpack2(t[3], o[6], o[7]);
  } else if constexpr (V == 4) {
    const rb_u32x2 t = ld_pol<NT>(reinterpret_cast<const rb_u32x2*>(p));
    unpack2(t[0], o[0], o[1]); unpack2(t[1], o[2], o[3]);
  } else if constexpr (V == 2) {
    unpack2(ld_pol<NT>(reinterpret_cast<const uint32_t*>(p)), o[0], o[1]);
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = (float)p[v];
  }
}

template <bool NT, int V>
__device__ __forceinline__ void st_b16(bf16_t* p, const float (&o)[V]) {
  if constexpr (V == 8) {
    st_pol<NT>(rb_u32x4{pack2(o[0], o[1]), pack2(o[2], o[3]), pack2(o[4], o[5]), pack2(o[6], o[7])},
               reinterpret_cast<rb_u32x4*>(p));
  } else if constexpr (V == 4) {
    st_pol<NT>(rb_u32x2{pack2(o[0], o[1]), pack2(o[2], o[3])}, reinterpret_cast<rb_u32x2*>(p));
  } else if constexpr (V == 2) {
    st_pol<NT>(pack2(o[0], o[1]), reinterpret_cast<uint32_t*>(p));
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) p[v] = (bf16_t)o[v];
  }
}

template <int V>
__device__ __forceinline__ void ldv(float (&o)[V], const bf16_t* p) { ld_b16<kNT>(o, p); }
template <int V>
__device__ __forceinline__ void stv(bf16_t* p, const float (&o)[V]) { st_b16<kNT>(p, o); }
template <int V>
__device__ __forceinline__ void ldc(float (&o)[V], const bf16_t* p) { ld_b16<false>(o, p); }
template <int V>
__device__ __forceinline__ void stc(bf16_t* p, const float (&o)[V]) { st_b16<false>(p, o); }

// raw (storage-format) register image of V elements: fp32 as is, bf16 as
// packed pairs, unpacked to fp32 only when used (prefetch buffers)
template <typename T, int V>
struct RawVec {
  float w[V];
};
template <int V>
struct RawVec<bf16_t, V> {
  static_assert(V % 2 == 0, "packed bf16 needs an even width");
  uint32_t w[V / 2];
};
template <>
struct RawVec<bf16_t, 1> {
  float w[1];
};

template <bool NT = kNT, int V>
__device__ __forceinline__ void ld_raw(RawVec<float, V>& o, const float* p) { ld_f32<NT>(o.w, p); }
template <int V>
__device__ __forceinline__ void unpack_raw(float (&o)[V], const RawVec<float, V>& r) {
#pragma unroll
  for (int v = 0; v < V; ++v) o[v] = r.w[v];
}
template <typename T, int V>
__device__ __forceinline__ void zero_raw(RawVec<T, V>& o) {
#pragma unroll
  for (int k = 0; k < (int)(sizeof(o.w) / sizeof(o.w[0])); ++k) o.w[k] = 0;
}

template <bool NT = kNT, int V>
__device__ __forceinline__ void ld_raw(RawVec<bf16_t, V>& o, const bf16_t* p) {
  if constexpr (V == 8) {
    const rb_u32x4 t = ld_pol<NT>(reinterpret_cast<const rb_u32x4*>(p));
    o.w[0] = t[0]; o.w[1] = t[1]; o.w[2] = t[2]; o.w[3] = t[3];
  } else if constexpr (V == 4) {
    const rb_u32x2 t = ld_pol<NT>(reinterpret_cast<const rb_u32x2*>(p));
    o.w[0] = t[0]; o.w[1] = t[1];
  } else if constexpr (V == 2) {
    o.w[0] = ld_pol<NT>(reinterpret_cast<const uint32_t*>(p));
  } else {
    o.w[0] = (float)p[0];
  }
}
template <int V>
__device__ __forceinline__ void unpack_raw(float (&o)[V], const RawVec<bf16_t, V>& r) {
  if constexpr (V == 1) {
    o[0] = r.w[0];
  } else {
#pragma unroll
    for (int k = 0; k < V / 2; ++k) unpack2(r.w[k], o[2 * k], o[2 * k + 1]);
  }
}

// channels h0 .. h0 + VH - 1 of a raw image (h0 even for packed bf16), and
// the reverse: VH results into a storage-format image (bf16: RNE pairs, as
// stv); stv_raw stores a whole image with stv's policy
template <int VH, typename T, int V>
__device__ __forceinline__ void unpack_part(float (&o)[VH], const RawVec<T, V>& r, int h0) {
  if constexpr (VH == V) {
    unpack_raw(o, r);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int v = 0; v < VH; ++v) o[v] = r.w[h0 + v];
  } else {
#pragma unroll
    for (int k = 0; k < VH / 2; ++k) unpack2(r.w[h0 / 2 + k], o[2 * k], o[2 * k + 1]);
  }
}
template <int VH, typename T, int V>
__device__ __forceinline__ void pack_part(RawVec<T, V>& r, const float (&o)[VH], int h0) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int v = 0; v < VH; ++v) r.w[h0 + v] = o[v];
  } else {
    static_assert(VH % 2 == 0, "packed bf16 pairs");
#pragma unroll
    for (int k = 0; k < VH / 2; ++k) r.w[h0 / 2 + k] = pack2(o[2 * k], o[2 * k + 1]);
  }
}
// the words of channels h0 .. h0 + VH - 1 through an empty volatile asm (an
// ordering point for the compiler; no instruction)
template <int VH, typename T, int V>
__device__ __forceinline__ void opaque_part(RawVec<T, V>& r, int h0) {
  constexpr int per = sizeof(T) == 2 && V > 1 ? 2 : 1;   // channels per word
#pragma unroll
  for (int k = 0; k < VH / per; ++k) asm volatile("" : "+v"(r.w[h0 / per + k]));
}
template <int V>
__device__ __forceinline__ void stv_raw(float* p, const RawVec<float, V>& r) { st_f32<kNT>(p, r.w); }
template <int V>
__device__ __forceinline__ void stv_raw(bf16_t* p, const RawVec<bf16_t, V>& r) {
  if constexpr (V == 8) {
    st_pol<kNT>(rb_u32x4{r.w[0], r.w[1], r.w[2], r.w[3]}, reinterpret_cast<rb_u32x4*>(p));
  } else if constexpr (V == 4) {
    st_pol<kNT>(rb_u32x2{r.w[0], r.w[1]}, reinterpret_cast<rb_u32x2*>(p));
  } else {
    static_assert(V == 2, "packed bf16 image");
    st_pol<kNT>(r.w[0], reinterpret_cast<uint32_t*>(p));
  }
}

// ---- dropout keep-flags ------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter = element index / 4, key =
// 64-bit seed, 4 uniform u32 per call -> keep flags of 4 consecutive elements.
// (each round's two 32 x 32 -> 64 products as one v_mad_u64_u32 each, not a
// v_mul_lo_u32 + v_mul_hi_u32 pair: the same bits in half the quarter-rate
// instructions — the dropout epilogues are bound by this VALU work)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
    const uint32_t lo0 = (uint32_t)p0, hi0 = (uint32_t)(p0 >> 32);
    const uint32_t lo1 = (uint32_t)p1, hi1 = (uint32_t)(p1 >> 32);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// Dropout of one tensor: no-op, an explicit uint8 keep-mask laid out like the
// data, or a Philox stream regenerated on demand (forward and backward see
// the same flags for the same element index).  mode is launch-uniform.
struct DropSpec {
  const uint8_t* mask;
  uint32_t key0, key1, keep_thresh;
  float scale;
  int mode;   // 0 none, 1 mask, 2 philox

  // multipliers (0 or scale) for elements e .. e+3, e % 4 == 0
  __device__ __forceinline__ void get4(int64_t e, float (&m)[4]) const {
    if (mode == 0) {
      m[0] = m[1] = m[2] = m[3] = 1.0f;
    } else if (mode == 1) {
      const uchar4 t = *reinterpret_cast<const uchar4*>(mask + e);
      m[0] = t.x * scale; m[1] = t.y * scale; m[2] = t.z * scale; m[3] = t.w * scale;
    } else {
      const uint64_t g = (uint64_t)e >> 2;
      const uint4 r = philox4x32_10(make_uint4((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u), key0,
                                    key1);
      m[0] = r.x < keep_thresh ? scale : 0.0f;
      m[1] = r.y < keep_thresh ? scale : 0.0f;
      m[2] = r.z < keep_thresh ? scale : 0.0f;
      m[3] = r.w < keep_thresh ? scale : 0.0f;
    }
  }
};

DropSpec make_drop(const uint8_t* mask, uint64_t seed, float p);

// ---- channel-last wave layout ---------------------------------------------------
// The [B, L, H] kernels give each wave one batch row b and a span of G*VEC
// channels.  Lane = q * G + g: g picks VEC consecutive channels (so the G lanes
// of one chunk read one contiguous G*VEC*4-byte segment of a row), q picks one
// of Q consecutive time chunks of TC steps inside a tile of Q*TC steps.
// Summaries of the Q chunks are combined across lanes with shuffles at stride
// G; no LDS and no barriers.

// host launch helpers (defined in the .hip files)
int launch_pack_plan(const int64_t* seq, int64_t seq_rs, const int64_t* offs,
                     const int64_t* order, int64_t B, int64_t* ids, int64_t* pos, int64_t* inv,
                     int64_t* last, hipStream_t st);
int launch_next_item_targets(const int64_t* ids, const int64_t* offs, const int64_t* order,
                             const int64_t* pos_items, int64_t B, int64_t ntok, int64_t m_pad,
                             int64_t* tgt, hipStream_t st);
// the recurrence launchers exist for T = float and T = bf16_t activation
// storage (explicit instantiations in scan_rows.hip, conv_silu.hip, gate_scan.hip)
template <typename T>
int launch_scan_fwd(const T* gates, const T* tokens, T* states, int64_t rows, int64_t steps,
                    hipStream_t st);
template <typename T>
int launch_scan_bwd(const T* gates, const T* states, const T* grad, T* d_gates, T* d_tokens,
                    int64_t rows, int64_t steps, hipStream_t st);
template <typename T>
int launch_conv_fwd(const T* x, int64_t x_rs, const float* w, const float* bias, T* xc,
                    int64_t xc_rs, int64_t B, int64_t L, int64_t H, int64_t K,
                    const int64_t* offs, hipStream_t st);
template <typename T>
int launch_conv_fwd_rows(const T* x, int64_t x_rs, const float* w, const float* bias, T* xc,
                         int64_t xc_rs, int64_t ntok, int64_t H, int64_t K, const int64_t* pos,
                         hipStream_t st);
template <typename T>
int launch_conv_bwd(const T* x, int64_t x_rs, const float* w, const float* bias, const T* g1,
                    const T* g2, T* dx, int64_t dx_rs, float* dw_part, float* db_part, int64_t B,
                    int64_t L, int64_t H, int64_t K, const int64_t* offs, hipStream_t st);
// y_last / dy_last [B, H] (rows permuted by order): rb_gate_scan_*_last;
// z_last / dz_last [B, H] (rows likewise, fp32): their sparse-z mode, z and dz unused
template <typename T>
int launch_gate_fwd(const T* rg, int64_t rg_rs, const T* xc, int64_t xc_rs, const T* z,
                    int64_t z_rs, const float* lam, const float* gb, const float* h0,
                    int64_t h0_bs, T* y, int64_t y_rs, float* carries, int64_t B, int64_t L,
                    int64_t H, const int64_t* offs, hipStream_t st, T* y_last = nullptr,
                    const int64_t* order = nullptr, const T* z_last = nullptr);
template <typename T>
int launch_gate_bwd(const T* rg, int64_t rg_rs, const T* xc, int64_t xc_rs, const T* z,
                    int64_t z_rs, const float* lam, const float* gb, const float* carries,
                    const T* dy, T* drg, int64_t drg_rs, T* dxc, int64_t dxc_rs, T* dz,
                    int64_t dz_rs, float* part, float* dh0_part, int64_t B, int64_t L, int64_t H,
                    const int64_t* offs, hipStream_t st, const T* dy_last = nullptr,
                    const int64_t* order = nullptr, const T* z_last = nullptr,
                    T* dz_last = nullptr);
int launch_add_ln_fwd(const float* a, const int64_t* idx, int64_t nidx, const DropSpec& drop,
                      const float* r, const float* gamma, const float* beta, float eps, float* y,
                      float* s_out, float* mean, float* rstd, int64_t rows, int64_t d,
                      hipStream_t st);
int launch_add_ln_bwd(const float* dy, const float* dy2, const float* s, const float* gamma,
                      const float* mean, const float* rstd, const DropSpec& drop, float* ds,
                      float* da, float* dgp, float* dbp, float* dbiasp, int64_t nparts,
                      int64_t rows, int64_t d, hipStream_t st);
int64_t ln_num_parts(int64_t rows, int64_t d);
int launch_silu_dropout_fwd(const float* a, const float* bias, const DropSpec& drop, float* u,
                            int64_t rows, int64_t cols, hipStream_t st);
int launch_silu_dropout_bwd(const float* a, const float* bias, const DropSpec& drop,
                            const float* du, float* da, float* dbias_part, int64_t nparts,
                            int64_t rows, int64_t cols, hipStream_t st);
int launch_dropout_mask(const DropSpec& drop, uint8_t* out, int64_t n, hipStream_t st);
int launch_split_weights_h(const rb_split_job* jobs, int n, hipStream_t st);
int launch_bf16_weight_image(const float* W, int64_t ldw, int C, int R, int transpose, void* img,
                             hipStream_t st);
int launch_gemm_nt_bf16(const void* A, int64_t lda, int64_t M, int R, const void* img, int C,
                        const float* bias, void* out, int64_t ldo, hipStream_t st);
int launch_gemm_tn_h(const float* Y, int64_t ldy, const float* X, int64_t ldx, int64_t M, int N,
                     int K, const float* ymax, const float* xmax, float* parts, int S,
                     hipStream_t st);
// ---- the f16 weight image -----------------------------------------------------
// The image of Bm [C, R] (Bm = W, or W^T with transpose) that
// k_split_weights_h (gemm_half.hip) writes and every f16x3 kernel with a
// weight operand reads (rb_gemm_h_weight_bytes), three parts:
//   * the 32-column planes at byte 0, v_mfma_f32_32x32x16_f16 operand order:
//     16-B slot weight_slot32(R / 16, cb, kb, p, lane) = plane p (0 hi, 1 lo)
//     of Bm[32 cb + lane % 32][16 kb + 8 (lane / 32) + 0..7] * 2^(kWeightScale - e_c);
//   * the column exponents at byte C * R * 4: int32 e_c, the frexp exponent
//     of max_r |Bm[c, r]| (0 for an all-zero column), so every scaled column
//     max lies in [2^(kWeightScale - 1), 2^kWeightScale);
//   * the 16-column planes at byte ws_image_offset(C, R) (only when
//     R % 32 == 0), v_mfma_f32_16x16x32_f16 operand order: slot
//     weight_slot16(R / 32, cb, ks, p, lane) = plane p of
//     Bm[16 cb + lane % 16][32 ks + 8 (lane / 16) + 0..7], same scale.
// A reader un-scales with e_c - kWeightScale, so writer and readers share
// the one constant.
constexpr int kWeightScale = 14;
// a 16-B slot (in units of 16 B from its planes' start) and the column and
// first k of the 8 values it holds.  S, the slot's type, and I, the type
// the block index cb * nkb + kb is formed in, only choose the width of a
// caller's address arithmetic: int64_t S for a whole image, int for an
// offset inside a few column blocks (the formulas are linear, so an address
// may be formed as slot(cb, 0, 0, lane) + slot(0, kb, p, 0)).
template <class S>
struct WeightSlot {
  S slot;
  int col, k0;
};
// nkb: the k-blocks of a column block (R / 16, R / 32)
template <class S = int64_t, class I>
__host__ __device__ inline WeightSlot<S> weight_slot32(int nkb, I cb, int kb, int p, int lane) {
  return {((S)(cb * nkb + kb) * 2 + p) * 64 + lane, (int)cb * 32 + (lane & 31),
          kb * 16 + 8 * (lane >> 5)};
}
template <class S = int64_t, class I>
__host__ __device__ inline WeightSlot<S> weight_slot16(int nkb, I cb, int ks, int p, int lane) {
  return {((S)(cb * nkb + ks) * 2 + p) * 64 + lane, (int)cb * 16 + (lane & 15),
          ks * 32 + 8 * (lane >> 4)};
}
// byte offset of the 16-column planes (after the 32-column planes and the
// exponents)
__host__ __device__ inline int64_t ws_image_offset(int64_t C, int64_t K) {
  return C * K * 4 + ((C * 4 + 15) / 16) * 16;
}
// The three parts of an image Wf.
struct WeightImage {
  const void* wf;
  const int* ew;
  const void* wi;
};
inline WeightImage weight_image(const void* Wf, int64_t C, int64_t R) {
  const char* base = static_cast<const char*>(Wf);
  return {Wf, reinterpret_cast<const int*>(base + C * R * 4), base + ws_image_offset(C, R)};
}
// zeroes dpart's rows [used, n_parts) (both rb_gemm_nt_h_dact kernels)
int nt_dact_zero_rest(float* dpart, int64_t used, int64_t n_parts, int C, hipStream_t st);
bool nt_ws_ok(int64_t M, int K, int C, const float* A, int64_t lda, const float* out, int64_t ldo);
int launch_gemm_nt_ws(const float* A, int64_t lda, int64_t M, int K, const void* Wf, int C,
                      const float* bias, float* out, int64_t ldo, float* rmax, hipStream_t st);
int gemm_nt_h_mode(int mode);
bool nt_ws_act_ok(int64_t M, int K, int C, const float* A, int64_t lda, const float* out,
                  const float* other, int64_t ldo);
int launch_gemm_nt_ws_act(const float* A, int64_t lda, int64_t M, int K, const void* Wf, int C,
                          const float* bias, float* out, int64_t ldo, float* rmax, float* act,
                          DropSpec drop, hipStream_t st);
int launch_gemm_nt_ws_dact(const float* A, int64_t lda, int64_t M, int K, const void* Wf, int C,
                           float* out, int64_t ldo, float* rmax, const float* pre, DropSpec drop,
                           float* dpart, int64_t n_parts, hipStream_t st);
bool nt_ws_ln_ok(int64_t M, int K, int C, const float* A, int64_t lda, const float* y,
                 const float* s_out, const float* resid, int64_t ldo);
int launch_gemm_nt_ws_ln(const float* A, int64_t lda, int64_t M, int K, const void* Wf, int C,
                         const float* bias, const float* resid, DropSpec drop, const float* gamma,
                         const float* beta, float eps, float* y, float* s_out, float* mean,
                         float* rstd, int64_t ldo, float* rmax, hipStream_t st);
int launch_gemm_nt_h(const float* A, int64_t lda, int64_t M, int R, const void* Wf, int C,
                     const float* bias, float* out, int64_t ldo, int accumulate, float* rmax,
                     hipStream_t st);
int launch_gemm_nt_h_act(const float* A, int64_t lda, int64_t M, int R, const void* Wf, int C,
                         const float* bias, float* out, int64_t ldo, float* rmax, float* act,
                         DropSpec drop, hipStream_t st);
int64_t nt_h_dact_parts();
int launch_gemm_nt_h_dact(const float* A, int64_t lda, int64_t M, int R, const void* Wf, int C,
                          float* out, int64_t ldo, float* rmax, const float* pre, DropSpec drop,
                          float* dpart, int64_t n_parts, hipStream_t st);
int launch_adam(const rb_adam_job* jobs, int n, double lr, double beta1, double beta2, double eps,
                double weight_decay, double bc1, double bc2, hipStream_t st);
int launch_gemm_nt_hs(const float* A, int64_t lda, int64_t M, int R, const void* Wf, int C,
                      const float* bias, float* out, int64_t ldo, float* rmax, hipStream_t st);
int launch_gemm_tn_hs(const float* Y, int64_t ldy, const float* X, int64_t ldx, int64_t M, int N,
                      int K, float* dw, int accumulate, hipStream_t st);
int64_t emb_workspace_bytes(int64_t M, int64_t V, int64_t d);
int launch_embedding_plan(const int64_t* idx, int64_t M, int64_t d, int64_t V, void* workspace,
                          int64_t ws_bytes, hipStream_t st);
int launch_embedding_apply(const float* grad, int64_t M, int64_t d, int64_t V,
                           int64_t padding_idx, float* dw, void* workspace, int64_t ws_bytes,
                           hipStream_t st);
int launch_embedding_bwd(const int64_t* idx, const float* grad, int64_t M, int64_t d, int64_t V,
                         int64_t padding_idx, float* dw, void* workspace, int64_t ws_bytes,
                         hipStream_t st);
int launch_embedding_apply_scaled(const float* src, int64_t src_ld, int64_t src_rows,
                                  const float* coef, int64_t M, int64_t d, int64_t V,
                                  int64_t padding_idx, float* dw, void* workspace,
                                  int64_t ws_bytes, hipStream_t st);
int launch_sample_negatives(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                            const int64_t* pos_items, const int64_t* offsets, const int64_t* inv,
                            int64_t B, int64_t L, int64_t n_neg, int64_t first, int64_t V,
                            uint64_t seed, int64_t ntok, int64_t m_pad, const int64_t* alias,
                            int64_t* neg, hipStream_t st);   // alias: NULL = uniform
int64_t pair_loss_workspace_bytes(int64_t M);
int launch_pair_loss_fwd(const float* h, int64_t ldh, const float* tab, const int64_t* pos,
                         const int64_t* neg, int64_t M, int64_t d, int64_t V, int64_t n_neg,
                         float gamma, float* diff, float* loss, int64_t* n_live, void* workspace,
                         hipStream_t st);
int launch_pair_loss_bwd(const float* tab, const int64_t* pos, const int64_t* neg,
                         const float* diff, const float* dloss, const int64_t* n_live, int64_t M,
                         int64_t d, int64_t V, int64_t n_neg, float gamma, float* dh, float* coef,
                         hipStream_t st);
int64_t shared_softmax_blocks(int64_t B, int64_t max_len);
int64_t shared_softmax_workspace_bytes(int64_t B, int64_t max_len);
int launch_shared_softmax_fwd(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                              const int64_t* neg, const int64_t* offsets, const int64_t* order,
                              int64_t M, int64_t B, int64_t d, int64_t V, int64_t n,
                              int64_t max_len, float shift, const float* item_shift, float* lse,
                              float* z0, float* loss, int64_t* n_live, void* workspace,
                              hipStream_t st);   // item_shift: NULL = the scalar shift only
int launch_shared_softmax_bwd(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                              const int64_t* neg, const int64_t* offsets, const int64_t* order,
                              const float* lse, const float* dloss, const int64_t* n_live,
                              int64_t M, int64_t B, int64_t d, int64_t V, int64_t n,
                              int64_t max_len, float shift, const float* item_shift, float* dh,
                              float* coef, float* dneg, hipStream_t st);
int launch_candidate_scores(const float* h, int64_t ldh, const float* tab, const int64_t* cand,
                            int64_t B, int64_t C, int64_t d, int64_t V, float* scores,
                            hipStream_t st);
int launch_candidate_topk(const float* h, int64_t ldh, const float* tab, const int64_t* cand,
                          int64_t B, int64_t C, int64_t d, int64_t V, int64_t first, int64_t k,
                          const int64_t* exclude, int64_t E, int64_t* ids, float* scores,
                          hipStream_t st);
int64_t candidate_rank_chunks(int64_t C);
int launch_candidate_ranks(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                           const int64_t* cand, int64_t B, int64_t C, int64_t d, int64_t V,
                           int64_t first, int64_t* n_gt, int64_t* n_eq, hipStream_t st);
int64_t item_ce_workspace_bytes(int64_t B, int64_t V, int64_t D);
int64_t item_rank_workspace_bytes(int64_t B, int64_t V);
int launch_item_ce_fwd(const float* E, const float* W, const int64_t* tgt, int64_t B, int64_t V,
                       int64_t D, float* lse, float* loss, void* ws, int64_t ws_bytes,
                       hipStream_t st);
int launch_item_ce_bwd(const float* E, const float* W, const int64_t* tgt, const float* lse,
                       const float* dloss, int64_t B, int64_t V, int64_t D, float* dE, float* dW,
                       void* ws, int64_t ws_bytes, hipStream_t st);
// The options of the fused top-k and ranks, as the kernels take them.  A launch
// function takes each by pointer, null where the option is off.
// Allow-bitmaps (include/recblr_filters.h): words [F, W] int32 (bit i of word w
// of filter f: item 32 w + i is allowed), rows [B] int64 or null: the filter
// each row selects.
struct AllowArgs {
  const int* words;
  int64_t F, W;
  const int64_t* rows;
};
// Diversity caps (include/recblr_groups.h): at most m items of a group per list.
struct GroupArgs {
  const int* ids;   // [V], -1 (uncapped) or a group in [0, RB_GROUP_ID_MAX]
  int m;
};
// Score priors (include/recblr_priors.h): values [P, V] fp32, rows [B] int64 or
// null (the prior each row takes), weight [B] fp32 or null (1 for every row).
struct PriorArgs {
  const float* values;
  int64_t P, V;
  const int64_t* rows;
  const float* weight;
};
// fn: the C entry point's name, for the messages.  The top-k workspace is the
// grouped one's with gr, the plain one's without.
int launch_item_rank(const char* fn, const float* E, const float* W, const int64_t* tgt,
                     int64_t B, int64_t V, int64_t D, int64_t first, int64_t* n_gt,
                     int64_t* n_eq, void* ws, int64_t ws_bytes, const AllowArgs* al,
                     const PriorArgs* pa, hipStream_t st);
int64_t item_topk_workspace_bytes(int64_t B, int64_t V, int64_t k);
int64_t item_topk_grouped_workspace_bytes(int64_t B, int64_t V, int64_t k);
int launch_item_topk(const char* fn, const float* E, const float* W, int64_t B, int64_t V,
                     int64_t D, int64_t k, int64_t first, const int64_t* ex, int64_t NE,
                     int64_t* ids, float* scores, void* ws, int64_t ws_bytes,
                     const AllowArgs* al, const GroupArgs* gr, const PriorArgs* pa,
                     hipStream_t st);
int launch_item_ce_probs(const float* E, const float* W, const int64_t* tgt, const float* lse,
                         const float* dloss, int64_t B, int64_t V, int64_t D, int64_t v_off,
                         float* out, int64_t ld, hipStream_t st);
int launch_item_scores(const float* E, const float* W, int64_t B, int64_t V, int64_t D,
                       float* out, hipStream_t st);
int launch_item_split_h(const float* X, int64_t N, int64_t D, void* img, int* ex, float* gmax,
                        hipStream_t st);
int launch_item_ce_fwd_h(const void* Ei, const int* Ee, const void* Wi, const int* We,
                         const int64_t* tgt, int64_t B, int64_t V, int64_t D, float* lse,
                         float* loss, void* ws, int64_t ws_bytes, bool rows_mode, float inv_n,
                         int accumulate, hipStream_t st);
// What rb_item_ce_probs_h* writes.  p: P [B, ld]; pt: P^T [V, ldt]; either may
// be null, and with both set row_max / item_max take every 32-row / 32-item
// group's max |P| (item_max alone goes with pt alone).  rows: a target of -1 is
// an ignored row and P is scaled by inv_n, not by 1 / B.
struct CeProbsOut {
  float* p;
  int64_t ld;
  float* pt;
  int64_t ldt;
  float* row_max;
  float* item_max;
  bool rows;
  float inv_n;
};
int launch_item_ce_probs_h(const void* Ei, const int* Ee, const void* Wi, const int* We,
                           const int64_t* tgt, const float* lse, const float* dloss, int64_t B,
                           int64_t V, int64_t D, int64_t v_off, const CeProbsOut& o,
                           hipStream_t st);
int launch_group_absmax(const float* x, int64_t n, int64_t c, int64_t ld, float* out,
                        hipStream_t st);
int launch_pad_prefix_fwd(const float* conv_b, const float* gw, const float* gb,
                          const float* lam, const int64_t* pad, int64_t pad_len, int64_t n_rows,
                          int64_t H, float* h0, float* ws, hipStream_t st);
int launch_pad_prefix_bwd(const float* conv_b, const float* gw, const float* gb,
                          const float* lam, const int64_t* pad, int64_t pad_len, int64_t n_rows,
                          int64_t H, const float* dh0, float* dconv_b, float* dgw, float* dgb,
                          float* dlam, float* ws, int accumulate, hipStream_t st);
int launch_colsum(const float* in, int64_t M, int64_t P, int64_t C, int64_t rs, int64_t ms,
                  float* out, hipStream_t st);
int launch_colsum_chunked(const float* in, int64_t M, int64_t P, int64_t C, int64_t rs, int CH,
                          float* part, unsigned* cnt, float* out, hipStream_t st);

}  // namespace rb

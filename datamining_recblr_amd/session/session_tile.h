// session_tile.h — what the session kernels share (session_step.hip,
// session_append.hip): one workgroup carries RB_SESSION_TILE = 16 rows through
// the embedding LayerNorm and every layer.  The 16 rows are the M of the
// exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), every weight matrix is streamed
// once per workgroup as the B operand straight from global memory (L2 / MALL
// after the first workgroup), and the activations live in three LDS buffers:
//   xs [16][d]              the layer input / residual / result
//   as [16][2H]             u | z, then xc | z, then y | z; later the w_2 output
//   gs [16][max(2H, 4d)]    r | i, then the out-projection, then the FFN hidden
// followed by the 16 rows' meta (slot, item, flag).
//
// Determinism: a row's values are a function of that row alone.  D[i][j] of
// the MFMA is a k-ordered fma chain over row i of A; the LayerNorm
// reductions run inside the 32 lanes that own a row; there are no atomics.
// So a row's results do not depend on its position in the tile, on the
// other rows, or on B: the step's 16 rows are 16 slots, the append's are T
// consecutive events of 16 / T slots, and both compute the same bits.
#ifndef RECBLR_SESSION_TILE_H
#define RECBLR_SESSION_TILE_H

#include "../csrc/common.h"
#include "recblr_session.h"

namespace rb {

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = RB_SESSION_TILE;
constexpr int kRowLanes = kThreads / kTile;   // 32 threads own a row in the LayerNorms
constexpr int kPad = 4;                       // floats of padding per LDS row
constexpr int kMetaBytes = kTile * (8 + 8 + 4);

// row flags; the append kernel keeps its call row's event count above them
enum : int { kValid = 1, kFresh = 2, kCountShift = 8 };

// the kernels' argument block (y_all and T: the append kernel only)
struct TileArgs {
  rb_session_layer layer[RB_SESSION_MAX_LAYERS];
  const float* emb;
  const float* ln_w;
  const float* ln_b;
  const int64_t* items;
  const int64_t* slots;
  int64_t* count;
  float* out;
  float* y;
  float* y_all;
  int32_t* status;
  int64_t B, N, V;
  float eps;
  int n_layers, d, H, K, use_conv, use_ffn, T;
};

__host__ __device__ inline int g_width(int d, int H) { return 2 * H > 4 * d ? 2 * H : 4 * d; }

inline int64_t tile_lds_bytes(int64_t d, int64_t H) {
  return (int64_t)kTile * (d + 2 * H + g_width((int)d, (int)H) + 3 * kPad) * 4 + kMetaBytes;
}

// the LDS plan: three activation buffers with their row strides, then the meta
struct TileLds {
  float *xs, *as, *gs;
  int64_t *slot, *item;
  int* flag;
  int ldx, lda, ldg;
};

__device__ __forceinline__ TileLds tile_lds(char* smem, int d, int H) {
  TileLds s;
  s.ldx = d + kPad;
  s.lda = 2 * H + kPad;
  s.ldg = g_width(d, H) + kPad;
  s.xs = reinterpret_cast<float*>(smem);
  s.as = s.xs + kTile * s.ldx;
  s.gs = s.as + kTile * s.lda;
  s.slot = reinterpret_cast<int64_t*>(s.gs + kTile * s.ldg);
  s.item = s.slot + kTile;
  s.flag = reinterpret_cast<int*>(s.item + kTile);
  return s;
}

// U 16-wide k blocks of two 16-column tiles: all 3U 16-byte loads are issued
// before the first MFMA, so a wave keeps 2U weight loads in flight (the step
// is bound by the latency of streaming W, not by the MFMA rate).
template <int U>
__device__ __forceinline__ void mfma_blocks(const float* xa, const float* __restrict__ w0,
                                            const float* __restrict__ w1, rb_f32x4& acc0,
                                            rb_f32x4& acc1) {
  rb_f32x4 a[U], b0[U], b1[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    b0[u] = *reinterpret_cast<const rb_f32x4*>(w0 + 16 * u);
    b1[u] = *reinterpret_cast<const rb_f32x4*>(w1 + 16 * u);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) a[u] = *reinterpret_cast<const rb_f32x4*>(xa + 16 * u);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b0[u][j], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b1[u][j], acc1, 0, 0, 0);
    }
  }
}

// Ys[16][N] = Xs[16][Kd] W^T; W [N, Kd] row-major in global memory, Xs / Ys in
// LDS.  A wave computes two 16-column tiles per pass from one A fragment (the
// second is a copy of the first where N has no second tile for the wave).
// Each lane reads 4 consecutive k of its row (16 B) of A and of W, so MFMA j
// of a 16-wide k block sums k = kb + 4 (lane >> 4) + j: a permuted but fixed
// k order, the same for every row.
__device__ __forceinline__ void gemm16(const float* Xs, int ldx, const float* __restrict__ W,
                                       int Kd, int N, float* Ys, int ldy) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const float* xa = Xs + r * ldx + 4 * g;
  const int ntiles = N >> 4;
  for (int t = wave; t < ntiles; t += 2 * kWaves) {
    const bool two = t + kWaves < ntiles;   // wave-uniform
    const float* w0 = W + (int64_t)(t * 16 + r) * Kd + 4 * g;
    const float* w1 = two ? w0 + (int64_t)kWaves * 16 * Kd : w0;
    rb_f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
    int kb = 0;
    for (; kb + 128 <= Kd; kb += 128) mfma_blocks<8>(xa + kb, w0 + kb, w1 + kb, acc0, acc1);
    for (; kb + 64 <= Kd; kb += 64) mfma_blocks<4>(xa + kb, w0 + kb, w1 + kb, acc0, acc1);
    for (; kb < Kd; kb += 16) mfma_blocks<1>(xa + kb, w0 + kb, w1 + kb, acc0, acc1);
    // C/D: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int q = 0; q < 4; ++q) Ys[(4 * g + q) * ldy + t * 16 + r] = acc0[q];
    if (two) {
#pragma unroll
      for (int q = 0; q < 4; ++q) Ys[(4 * g + q) * ldy + (t + kWaves) * 16 + r] = acc1[q];
    }
  }
}

__device__ __forceinline__ float sum_row_lanes(float v) {
#pragma unroll
  for (int o = kRowLanes / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kRowLanes);
  return v;
}

// xs[m] = LayerNorm(xs[m] + (src[m] + bias)) for the 16 rows (src NULL: LayerNorm(xs[m])).
// Two-pass variance, as rownorm.hip; 32 lanes own a row.
__device__ __forceinline__ void row_ln(float* xs, int ldx, int d, const float* src, int lds,
                                       const float* __restrict__ bias,
                                       const float* __restrict__ gamma,
                                       const float* __restrict__ beta, float eps) {
  const int m = threadIdx.x / kRowLanes, sub = threadIdx.x % kRowLanes;
  float* row = xs + m * ldx;
  float s = 0.0f;
  for (int c = sub; c < d; c += kRowLanes) {
    float v = row[c];
    if (src != nullptr) {
      float t = src[m * lds + c];
      if (bias != nullptr) t = t + bias[c];
      v = t + v;
      row[c] = v;
    }
    s += v;
  }
  const float mean = sum_row_lanes(s) / (float)d;
  float q = 0.0f;
  for (int c = sub; c < d; c += kRowLanes) {
    const float t = row[c] - mean;
    q += t * t;
  }
  const float rs = 1.0f / sqrtf(sum_row_lanes(q) / (float)d + eps);
  for (int c = sub; c < d; c += kRowLanes) row[c] = (row[c] - mean) * rs * gamma[c] + beta[c];
}

// xs = LayerNorm(emb[item]) for the rows flagged valid, zeros into the LayerNorm
// for the others.  Ends synchronised.
__device__ __forceinline__ void embed_rows(const TileArgs& a, const TileLds& s) {
  const int d = a.d;
  for (int e = threadIdx.x; e < kTile * d; e += kThreads) {
    const int m = e / d, c = e - m * d;
    s.xs[m * s.ldx + c] = (s.flag[m] & kValid) ? a.emb[s.item[m] * d + c] : 0.0f;
  }
  __syncthreads();
  row_ln(s.xs, s.ldx, d, nullptr, 0, nullptr, a.ln_w, a.ln_b, a.eps);
  __syncthreads();
}

// The position-wise rest of a layer after the recurrence left y | z in as:
// xs = LN(y W_out^T + xs), then xs = LN(w_2 silu(w_1 xs + b_1) + b_2 + xs).
// Starts and ends synchronised.
__device__ __forceinline__ void layer_tail(const TileArgs& a, const rb_session_layer& L,
                                           const TileLds& s) {
  const int d = a.d, H = a.H;
  gemm16(s.as, s.lda, L.w_out, H, d, s.gs, s.ldg);
  __syncthreads();
  row_ln(s.xs, s.ldx, d, s.gs, s.ldg, nullptr, L.ln_w, L.ln_b, a.eps);
  __syncthreads();
  if (a.use_ffn) {
    gemm16(s.xs, s.ldx, L.w1, d, 4 * d, s.gs, s.ldg);
    __syncthreads();
    for (int e = threadIdx.x; e < kTile * 4 * d; e += kThreads) {
      const int m = e / (4 * d), c = e - m * 4 * d;
      s.gs[m * s.ldg + c] = fsilu(s.gs[m * s.ldg + c] + L.b1[c]);
    }
    __syncthreads();
    gemm16(s.gs, s.ldg, L.w2, 4 * d, d, s.as, s.lda);
    __syncthreads();
    row_ln(s.xs, s.ldx, d, s.as, s.lda, L.b2, L.ffn_ln_w, L.ffn_ln_b, a.eps);
    __syncthreads();
  }
}

// the argument block both launchers fill the same way
inline TileArgs tile_args(const rb_session_layer* layers, int n_layers, const float* emb,
                          const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                          const int64_t* slots, int64_t* count, float* out, float* y,
                          int32_t* status, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                          bool use_conv, bool use_ffn) {
  TileArgs a{};
  for (int i = 0; i < n_layers; ++i) a.layer[i] = layers[i];
  a.emb = emb; a.ln_w = ln_w; a.ln_b = ln_b;
  a.items = items; a.slots = slots; a.count = count; a.out = out; a.y = y; a.status = status;
  a.B = B; a.N = N; a.V = V;
  a.eps = eps;
  a.n_layers = n_layers; a.d = d; a.H = H; a.K = K;
  a.use_conv = use_conv; a.use_ffn = use_ffn;
  a.T = 1;
  return a;
}

}  // namespace

}  // namespace rb

#endif /* RECBLR_SESSION_TILE_H */

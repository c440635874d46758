// session_step.hip — the whole RecBLR encoder advanced by one event per
// session slot in one launch (recblr_session.h: rb_session_step).
//
// One workgroup owns RB_SESSION_TILE = 16 consecutive rows of the call and
// carries them through the embedding LayerNorm and every layer; the 16 rows
// are the M of the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), every weight
// matrix is streamed once per workgroup as the B operand straight from
// global memory (L2 / MALL after the first workgroup), and the activations
// live in three LDS buffers:
//   xs [16][d]              the layer input / residual / result
//   as [16][2H]             u | z, then xc | z, then y | z; later the w_2 output
//   gs [16][max(2H, 4d)]    r | i, then the out-projection, then the FFN hidden
// Only the slots' state (h, conv history), out, count, y and status are
// written to global memory, with ordinary vector stores.
//
// Determinism: a row's values are a function of that row alone.  D[i][j] of
// the MFMA is a k-ordered fma chain over row i of A; the LayerNorm
// reductions run inside the 32 lanes that own a row; there are no atomics.
// So a slot's results do not depend on its position in the tile, on the
// other rows, or on B.
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

enum : int { kValid = 1, kFresh = 2 };

struct StepArgs {
  rb_session_layer layer[RB_SESSION_MAX_LAYERS];
  const float* emb;
  const float* ln_w;
  const float* ln_b;
  const int64_t* items;
  const int64_t* slots;
  int64_t* count;
  float* out;
  float* y;
  int32_t* status;
  int64_t B, N, V;
  float eps;
  int n_layers, d, H, K, use_conv, use_ffn;
};

__host__ __device__ inline int g_width(int d, int H) { return 2 * H > 4 * d ? 2 * H : 4 * d; }

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

__global__ __launch_bounds__(kThreads) void k_session_step(const StepArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = a.d, H = a.H, K = a.K;
  const int ldx = d + kPad, lda = 2 * H + kPad, ldg = g_width(d, H) + kPad;
  float* xs = reinterpret_cast<float*>(smem);
  float* as = xs + kTile * ldx;
  float* gs = as + kTile * lda;
  int64_t* s_slot = reinterpret_cast<int64_t*>(gs + kTile * ldg);
  int64_t* s_item = s_slot + kTile;
  int* s_flag = reinterpret_cast<int*>(s_item + kTile);
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * kTile;

  // every id is range-checked here, before any address is formed from it
  if (tid < kTile) {
    const int64_t b = b0 + tid;
    int64_t slot = -1, item = 0;
    int flag = 0;
    if (b < a.B) {
      int st = RB_SESSION_NO_EVENT;
      slot = a.slots != nullptr ? a.slots[b] : b;
      item = a.items[b];
      if (slot < 0 || slot >= a.N) {
        st = RB_SESSION_BAD_SLOT;
        slot = -1;
      } else if (item < 0 || item >= a.V) {
        st = RB_SESSION_BAD_ITEM;
      } else if (item != 0) {
        st = RB_SESSION_STEPPED;
        flag = kValid | (a.count[slot] == 0 ? kFresh : 0);
      }
      if (a.status != nullptr) a.status[b] = st;
    }
    s_slot[tid] = slot;
    s_item[tid] = item;
    s_flag[tid] = flag;
  }
  __syncthreads();
  int any = 0;
#pragma unroll
  for (int m = 0; m < kTile; ++m) any |= s_flag[m];

  if (any) {
    for (int e = tid; e < kTile * d; e += kThreads) {
      const int m = e / d, c = e - m * d;
      xs[m * ldx + c] = (s_flag[m] & kValid) ? a.emb[s_item[m] * d + c] : 0.0f;
    }
    __syncthreads();
    row_ln(xs, ldx, d, nullptr, 0, nullptr, a.ln_w, a.ln_b, a.eps);
    __syncthreads();

    for (int li = 0; li < a.n_layers; ++li) {
      const rb_session_layer& L = a.layer[li];
      gemm16(xs, ldx, L.w_in, d, 2 * H, as, lda);
      __syncthreads();
      if (a.use_conv) {
        // xc = silu(conv_b + sum_j w[:, j] hist[j] + w[:, K-1] u), in place over u;
        // the history moves up one row and takes u
        for (int e = tid; e < kTile * H; e += kThreads) {
          const int m = e / H, c = e - m * H;
          const int flag = s_flag[m];
          if (!(flag & kValid)) continue;
          const float u = as[m * lda + c];
          float* hist = L.conv_state + s_slot[m] * (K - 1) * H + c;
          const float* w = L.conv_w + c * K;
          float acc = L.conv_b[c];
          for (int j = 0; j < K - 1; ++j) {
            const float hj = (flag & kFresh) ? 0.0f : hist[(int64_t)j * H];
            acc += w[j] * hj;
            if (j > 0) hist[(int64_t)(j - 1) * H] = hj;
          }
          acc += w[K - 1] * u;
          if (K > 1) hist[(int64_t)(K - 2) * H] = u;
          as[m * lda + c] = fsilu(acc);
        }
        __syncthreads();
      }
      gemm16(as, lda, L.w_gate, H, 2 * H, gs, ldg);
      __syncthreads();
      // gates, one recurrence step, y = silu(z) h in place over xc
      for (int e = tid; e < kTile * H; e += kThreads) {
        const int m = e / H, c = e - m * H;
        const int flag = s_flag[m];
        if (!(flag & kValid)) continue;
        const float r = gs[m * ldg + c] + L.b_gate[c];
        const float i = gs[m * ldg + H + c] + L.b_gate[H + c];
        const float alpha = fexp(-softplus_f(L.lam[c]) * fsigm(r));
        const float beta = fsqrt(1.0f - alpha * alpha + 1e-8f) * fsigm(i);
        const float xc = as[m * lda + c];
        float* hp = L.h + s_slot[m] * H + c;
        const float h_in = (flag & kFresh) ? (L.h0 != nullptr ? L.h0[c] : 0.0f) : *hp;
        const float h = h_in * alpha + beta * xc;
        *hp = h;
        as[m * lda + c] = fsilu(as[m * lda + H + c]) * h;
      }
      __syncthreads();
      gemm16(as, lda, L.w_out, H, d, gs, ldg);
      __syncthreads();
      row_ln(xs, ldx, d, gs, ldg, nullptr, L.ln_w, L.ln_b, a.eps);
      __syncthreads();
      if (a.use_ffn) {
        gemm16(xs, ldx, L.w1, d, 4 * d, gs, ldg);
        __syncthreads();
        for (int e = tid; e < kTile * 4 * d; e += kThreads) {
          const int m = e / (4 * d), c = e - m * 4 * d;
          gs[m * ldg + c] = fsilu(gs[m * ldg + c] + L.b1[c]);
        }
        __syncthreads();
        gemm16(gs, ldg, L.w2, 4 * d, d, as, lda);
        __syncthreads();
        row_ln(xs, ldx, d, as, lda, L.b2, L.ffn_ln_w, L.ffn_ln_b, a.eps);
        __syncthreads();
      }
    }
  }

  // out[slot] = x for the rows that stepped; y[b] = the row's out either way
  for (int e = tid; e < kTile * d; e += kThreads) {
    const int m = e / d, c = e - m * d;
    const int64_t b = b0 + m, slot = s_slot[m];
    if (b >= a.B) continue;
    float v = 0.0f;
    if (s_flag[m] & kValid) {
      v = xs[m * ldx + c];
      a.out[slot * d + c] = v;
    } else if (slot >= 0) {
      v = a.out[slot * d + c];
    }
    if (a.y != nullptr) a.y[b * d + c] = v;
  }
  if (tid < kTile && (s_flag[tid] & kValid)) a.count[s_slot[tid]] += 1;
}

}  // namespace

int64_t session_lds_bytes(int64_t d, int64_t H) {
  return (int64_t)kTile * (d + 2 * H + g_width((int)d, (int)H) + 3 * kPad) * 4 + kMetaBytes;
}

int launch_session_step(const rb_session_layer* layers, int n_layers, const float* emb,
                        const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                        const int64_t* slots, int64_t* count, float* out, float* y,
                        int32_t* status, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                        bool use_conv, bool use_ffn, hipStream_t st) {
  StepArgs a{};
  for (int i = 0; i < n_layers; ++i) a.layer[i] = layers[i];
  a.emb = emb; a.ln_w = ln_w; a.ln_b = ln_b;
  a.items = items; a.slots = slots; a.count = count; a.out = out; a.y = y; a.status = status;
  a.B = B; a.N = N; a.V = V;
  a.eps = eps;
  a.n_layers = n_layers; a.d = d; a.H = H; a.K = K;
  a.use_conv = use_conv; a.use_ffn = use_ffn;
  const int lds = (int)session_lds_bytes(d, H);
  static bool done = false;  // benign race: idempotent
  if (!done) {
    (void)hipFuncSetAttribute((const void*)k_session_step,
                              hipFuncAttributeMaxDynamicSharedMemorySize, RB_SESSION_MAX_LDS);
    done = true;
  }
  const unsigned grid = (unsigned)((B + kTile - 1) / kTile);
  hipLaunchKernelGGL(k_session_step, dim3(grid), dim3(kThreads), lds, st, a);
  return launch_status("rb_session_step");
}

}  // namespace rb

// session_step.hip — the whole RecBLR encoder advanced by one event per
// session slot in one launch (recblr_session.h: rb_session_step).
//
// One workgroup owns RB_SESSION_TILE = 16 consecutive rows of the call, one
// slot per row, and carries them through the embedding LayerNorm and every
// layer (session_tile.h: the MFMA GEMM, the LayerNorms, the LDS plan).
// Only the slots' state (h, conv history), out, count, y and status are
// written to global memory, with ordinary vector stores.
#include "session_tile.h"

namespace rb {

namespace {

__global__ __launch_bounds__(kThreads) void k_session_step(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = a.d, H = a.H, K = a.K;
  const TileLds s = tile_lds(smem, d, H);
  float *xs = s.xs, *as = s.as, *gs = s.gs;
  int64_t *s_slot = s.slot, *s_item = s.item;
  int* s_flag = s.flag;
  const int ldx = s.ldx, lda = s.lda, ldg = s.ldg;
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
    embed_rows(a, s);

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
      layer_tail(a, L, s);
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

int64_t session_lds_bytes(int64_t d, int64_t H) { return tile_lds_bytes(d, H); }

int launch_session_step(const rb_session_layer* layers, int n_layers, const float* emb,
                        const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                        const int64_t* slots, int64_t* count, float* out, float* y,
                        int32_t* status, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                        bool use_conv, bool use_ffn, hipStream_t st) {
  const TileArgs a = tile_args(layers, n_layers, emb, ln_w, ln_b, eps, items, slots, count, out,
                               y, status, B, N, V, d, H, K, use_conv, use_ffn);
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

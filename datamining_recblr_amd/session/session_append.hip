// session_append.hip — up to 16 consecutive events per session slot in one
// launch (recblr_session.h: rb_session_append).
//
// Everything in the encoder is position-wise except the causal conv (it looks
// back K - 1 rows) and the recurrence (an elementwise serial chain).  So the
// 16 rows a workgroup carries (session_tile.h) are T consecutive events of
// 16 / T call rows: tile row r is event r % T of call row r / T.  The GEMMs,
// the LayerNorms and the FFN are the step's, row for row; the conv and the
// scan run one thread per (call row, channel) serially over that row's events,
// with the step's expressions in the step's order, so a slot is left bit for
// bit as rb_session_step per event would leave it.  The state (h, conv
// history, out, count) is written once, after the last event, with ordinary
// vector stores; a slot is written by one workgroup.
#include "session_tile.h"

namespace rb {

namespace {

__global__ __launch_bounds__(kThreads) void k_session_append(const TileArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = a.d, H = a.H, K = a.K, T = a.T;
  const int S = kTile / T;   // call rows of this tile
  const TileLds s = tile_lds(smem, d, H);
  float *xs = s.xs, *as = s.as, *gs = s.gs;
  int64_t *s_slot = s.slot, *s_item = s.item;
  int* s_flag = s.flag;
  const int ldx = s.ldx, lda = s.lda, ldg = s.ldg;
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * S;

  // Tile row tid looks at its whole call row: the events are the n entries
  // before the first 0, and every id is range-checked here, before any
  // address is formed from it.  flag = (n << kCountShift) | kValid | kFresh,
  // n = 0 for a masked row.
  if (tid < kTile) {
    const int sl = tid / T, t = tid - sl * T;
    const int64_t b = b0 + sl;
    int64_t slot = -1, item = 0;
    int flag = 0;
    if (b < a.B) {
      int st = RB_SESSION_NO_EVENT;
      slot = a.slots != nullptr ? a.slots[b] : b;
      if (slot < 0 || slot >= a.N) {
        st = RB_SESSION_BAD_SLOT;
        slot = -1;
      } else {
        const int64_t* row = a.items + b * T;
        int n = 0;
        bool bad = false;
        for (; n < T; ++n) {
          const int64_t v = row[n];
          if (v == 0) break;
          bad |= v < 0 || v >= a.V;
        }
        if (bad) {
          st = RB_SESSION_BAD_ITEM;
        } else if (n > 0) {
          st = RB_SESSION_STEPPED;
          flag = n << kCountShift;
          if (t < n) {
            item = row[t];
            flag |= kValid | (a.count[slot] == 0 ? kFresh : 0);
          }
        }
      }
      if (t == 0 && a.status != nullptr) a.status[b] = st;
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
        // Per (call row, channel): the K window in registers, right-aligned in
        // win[0..6] (its K - 1 history values end at win[6]); per event
        // xc = silu(conv_b + sum_j w[j] win[j] + w[K-1] u) in place over u,
        // then the window moves up and takes u.
        const int lo = 8 - K;   // first live entry of win and wr
        for (int e = tid; e < S * H; e += kThreads) {
          const int sl = e / H, c = e - sl * H, m0 = sl * T;
          const int flag = s_flag[m0];
          const int n = flag >> kCountShift;
          if (n == 0) continue;
          float* hist = K > 1 ? L.conv_state + s_slot[m0] * (K - 1) * H + c : nullptr;
          const float* w = L.conv_w + c * K;
          const float bias = L.conv_b[c], w_last = w[K - 1];
          float win[7], wr[7];
#pragma unroll
          for (int j = 0; j < 7; ++j) {
            const bool live = j >= lo;
            wr[j] = live ? w[j - lo] : 0.0f;
            win[j] = (live && !(flag & kFresh)) ? hist[(int64_t)(j - lo) * H] : 0.0f;
          }
          for (int t = 0; t < n; ++t) {
            const float u = as[(m0 + t) * lda + c];
            float acc = bias;
#pragma unroll
            for (int j = 0; j < 7; ++j)
              if (j >= lo) acc += wr[j] * win[j];
            acc += w_last * u;
            as[(m0 + t) * lda + c] = fsilu(acc);
#pragma unroll
            for (int j = 0; j < 6; ++j) win[j] = win[j + 1];
            win[6] = u;
          }
#pragma unroll
          for (int j = 0; j < 7; ++j)
            if (j >= lo) hist[(int64_t)(j - lo) * H] = win[j];
        }
        __syncthreads();
      }
      gemm16(as, lda, L.w_gate, H, 2 * H, gs, ldg);
      __syncthreads();
      // gates of every event, the recurrence serially over the call row's
      // events, y = silu(z) h in place over xc; h[slot] once at the end
      for (int e = tid; e < S * H; e += kThreads) {
        const int sl = e / H, c = e - sl * H, m0 = sl * T;
        const int flag = s_flag[m0];
        const int n = flag >> kCountShift;
        if (n == 0) continue;
        float* hp = L.h + s_slot[m0] * H + c;
        float h = (flag & kFresh) ? (L.h0 != nullptr ? L.h0[c] : 0.0f) : *hp;
        for (int t = 0; t < n; ++t) {
          const int m = m0 + t;
          const float r = gs[m * ldg + c] + L.b_gate[c];
          const float i = gs[m * ldg + H + c] + L.b_gate[H + c];
          const float alpha = fexp(-softplus_f(L.lam[c]) * fsigm(r));
          const float beta = fsqrt(1.0f - alpha * alpha + 1e-8f) * fsigm(i);
          const float xc = as[m * lda + c];
          h = h * alpha + beta * xc;
          as[m * lda + c] = fsilu(as[m * lda + H + c]) * h;
        }
        *hp = h;
      }
      __syncthreads();
      layer_tail(a, L, s);
    }
  }

  // y_all[b, t] = x after event t (zeros where there is none); out[slot] and
  // y[b] = x after the last event; y[b] = the stored out for a row without one
  for (int e = tid; e < kTile * d; e += kThreads) {
    const int m = e / d, c = e - m * d;
    const int sl = m / T, t = m - sl * T;
    const int64_t b = b0 + sl, slot = s_slot[m];
    if (b >= a.B) continue;
    const int flag = s_flag[m];
    const int n = flag >> kCountShift;
    const float v = (flag & kValid) ? xs[m * ldx + c] : 0.0f;
    if (a.y_all != nullptr) a.y_all[(b * T + t) * d + c] = v;
    if (n > 0 && t == n - 1) {
      a.out[slot * d + c] = v;
      if (a.y != nullptr) a.y[b * d + c] = v;
    } else if (n == 0 && t == 0 && a.y != nullptr) {
      a.y[b * d + c] = slot >= 0 ? a.out[slot * d + c] : 0.0f;
    }
  }
  if (tid < kTile && tid % T == 0) {
    const int n = s_flag[tid] >> kCountShift;
    if (n > 0) a.count[s_slot[tid]] += n;
  }
}

}  // namespace

int launch_session_append(const rb_session_layer* layers, int n_layers, const float* emb,
                          const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                          const int64_t* slots, int64_t* count, float* out, float* y,
                          float* y_all, int32_t* status, int64_t B, int T, int64_t N, int64_t V,
                          int d, int H, int K, bool use_conv, bool use_ffn, hipStream_t st) {
  TileArgs a = tile_args(layers, n_layers, emb, ln_w, ln_b, eps, items, slots, count, out, y,
                         status, B, N, V, d, H, K, use_conv, use_ffn);
  a.y_all = y_all;
  a.T = T;
  const int lds = (int)tile_lds_bytes(d, H);
  static bool done = false;  // benign race: idempotent
  if (!done) {
    (void)hipFuncSetAttribute((const void*)k_session_append,
                              hipFuncAttributeMaxDynamicSharedMemorySize, RB_SESSION_MAX_LDS);
    done = true;
  }
  const int rows = kTile / T;
  const unsigned grid = (unsigned)((B + rows - 1) / rows);
  hipLaunchKernelGGL(k_session_append, dim3(grid), dim3(kThreads), lds, st, a);
  return launch_status("rb_session_append");
}

}  // namespace rb

// session_capture.hip — the session state of a stored history, read off one
// layer's forward over the packed activations (recblr_session.h:
// rb_session_capture).
//
// The forward's gate scan checkpoints the recurrent state entering every
// RB_TILE-step tile (carries[b, tile, c], gate_scan.hip).  The state after a
// sequence's last position n - 1 is therefore the carry of tile (n - 1) /
// RB_TILE advanced by that tile's own 1 .. RB_TILE steps; the conv history
// is a copy of the last K - 1 pre-conv rows.
//
// Layout: a wave owns one packed sequence and 64 x 4 consecutive channels,
// four per lane (16-byte row pieces), as the other channel-last kernels do.
// The kernel is bound by latency: the addresses of the tile's steps do not
// depend on h, so all of them are loaded before the first step's arithmetic
// and alpha / b' of every step are formed ahead of the serial chain
// h = alpha h + b'.  No LDS, no barriers, no atomics; a slot is written by
// the one wave of its (sequence, channel span) with ordinary vector stores.
#include "../csrc/common.h"
#include "recblr_session.h"

namespace rb {

namespace {

constexpr int kVec = 4;
constexpr int kSpan = kWave * kVec;   // channels per wave

__global__ void __launch_bounds__(256)
k_session_capture(const float* __restrict__ u, int64_t u_rs, const float* __restrict__ xc,
                  int64_t xc_rs, const float* __restrict__ rg, int64_t rg_rs,
                  const float* __restrict__ lam, const float* __restrict__ gbias,
                  const float* __restrict__ carries, const int64_t* __restrict__ offs,
                  const int64_t* __restrict__ slots, float* __restrict__ h,
                  float* __restrict__ conv_state, int64_t B, int Lmax, int64_t N, int H, int K,
                  int ncw) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t b = wid / ncw;
  if (b >= B) return;   // wave-uniform, as every return below
  const int64_t row0 = offs[b];
  const int64_t n = offs[b + 1] - row0;
  // an empty sequence has no state to capture; one with more tiles than the
  // window has no carry row (carries is [B, ceil(Lmax / RB_TILE), H])
  const int nTc = (Lmax + RB_TILE - 1) / RB_TILE;   // carries row stride
  if (n < 1 || n > (int64_t)nTc * RB_TILE) return;
  const int64_t slot = slots[b];
  if (slot < 0 || slot >= N) return;   // before any address is formed from it
  const int c0 = (int)(wid - b * ncw) * kSpan + lane * kVec;
  if (c0 >= H) return;                 // channel tail (H % 4 == 0: whole vectors)

  const int tile = (int)((n - 1) / RB_TILE);
  const int64_t t0 = (int64_t)tile * RB_TILE;
  const int steps = (int)(n - t0);                  // 1 .. RB_TILE

  float nsp[kVec], br[kVec], bi[kVec], hv[kVec];
  ldc(nsp, lam + c0);
  ldc(br, gbias + c0);
  ldc(bi, gbias + H + c0);
  ldc(hv, carries + (b * nTc + tile) * H + c0);
  // every step's operands in flight at once (rows past the end: the last row
  // again, inside the sequence, and masked below)
  float r[RB_TILE][kVec], g[RB_TILE][kVec], x[RB_TILE][kVec];
#pragma unroll
  for (int s = 0; s < RB_TILE; ++s) {
    const int64_t row = row0 + t0 + min(s, steps - 1);
    ldc(r[s], rg + row * rg_rs + c0);
    ldc(g[s], rg + row * rg_rs + H + c0);
    ldc(x[s], xc + row * xc_rs + c0);
  }
#pragma unroll
  for (int v = 0; v < kVec; ++v) nsp[v] = -softplus_f(nsp[v]);
  // r <- alpha, x <- b' = beta * xc: the formula and operation order of
  // k_gate_scan_fwd (gate_scan.hip)
#pragma unroll
  for (int s = 0; s < RB_TILE; ++s) {
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
      const float a = fexp(nsp[v] * fsigm(r[s][v] + br[v]));
      const float beta = fsqrt(1.0f - a * a + 1e-8f) * fsigm(g[s][v] + bi[v]);
      r[s][v] = a;
      x[s][v] = beta * x[s][v];
    }
  }
#pragma unroll
  for (int s = 0; s < RB_TILE; ++s) {
    const bool ok = s < steps;   // steps past the end leave h as it is
#pragma unroll
    for (int v = 0; v < kVec; ++v) hv[v] = ok ? hv[v] * r[s][v] + x[s][v] : hv[v];
  }
  stc(h + slot * H + c0, hv);
  // the conv history: rows n - (K - 1) .. n - 1 of u, oldest first; zeros
  // stand for positions before the sequence's start.  After the recurrence,
  // whose registers are free by now: all K - 1 loads, then the stores
  if (conv_state != nullptr) {
    constexpr int kMaxHist = 7;   // K <= 8
    float row[kMaxHist][kVec];
#pragma unroll
    for (int k = 0; k < kMaxHist; ++k) {
#pragma unroll
      for (int v = 0; v < kVec; ++v) row[k][v] = 0.0f;
      const int64_t pos = n - (K - 1) + k;
      if (k < K - 1 && pos >= 0) ldc(row[k], u + (row0 + pos) * u_rs + c0);
    }
#pragma unroll
    for (int k = 0; k < kMaxHist; ++k)
      if (k < K - 1) stc(conv_state + (slot * (K - 1) + k) * H + c0, row[k]);
  }
}

}  // namespace

int launch_session_capture(const float* u, int64_t u_rs, const float* xc, int64_t xc_rs,
                           const float* rg, int64_t rg_rs, const float* lam, const float* gate_b,
                           const float* carries, const int64_t* offs, const int64_t* slots,
                           float* h, float* conv_state, int64_t B, int L, int64_t N, int H, int K,
                           hipStream_t st) {
  const int ncw = (H + kSpan - 1) / kSpan;
  const int64_t blocks = (B * ncw + 3) / 4;
  hipLaunchKernelGGL(k_session_capture, dim3((unsigned)blocks), dim3(256), 0, st, u, u_rs, xc,
                     xc_rs, rg, rg_rs, lam, gate_b, carries, offs, slots, h, conv_state, B, L, N,
                     H, K, ncw);
  return launch_status("rb_session_capture");
}

}  // namespace rb

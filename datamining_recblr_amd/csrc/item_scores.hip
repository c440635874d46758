// item_scores.hip — sequence representations scored against the item table on
// fp32 MFMA, without materialising the [B, V] logits:
//   * softmax cross-entropy over all items, forward and backward
//     (RecBLR.py:100-102: logits = seq_output @ item_embedding.weight^T,
//     nn.CrossEntropyLoss, mean over the batch);
//   * the rank of each row's target item among all items (the quantity the
//     full-sort Hit/NDCG/MRR@k evaluation reduces to, RecBLR.py:114-122 and
//     run_with_unseen.py:229-265);
//   * the plain score matrix (full_sort_predict itself).
//
// One wave computes 32 x 32 score tiles with v_mfma_f32_32x32x2_f32 over the
// full feature depth D; the 32-row operand that stays fixed over a wave's
// loop lives in registers, the other is streamed (L1/L2-resident: the item
// table is re-read by every row block).  Each lane owns the half
// k in [h*D/2, h*D/2 + D/2) of every row (h = lane / 32), so step s of the
// MFMA chain sums k = s (lanes 0-31) then k = D/2 + s (lanes 32-63).
// k_target_dot replays that exact fma chain, so a target's score is
// bit-identical to the score the tile kernels compute for it.
//
// An accumulator tile X has its column on the lane and its rows in the 16
// registers (row = (r&3) + 8(r>>2) + 4h), so X feeds the next MFMA as the
// operand summed over X's rows with no data movement: the CE backward uses
// P = softmax - onehot straight from the accumulators for dE = P W and
// dW = P^T E.  Every partial sum is written per split and reduced in a fixed
// order: results are deterministic.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "f16x3.h"

namespace rb {
namespace {

constexpr int kWaves = 4;            // waves per workgroup
constexpr int kTile = 32;            // rows (items or sequences) per wave tile
constexpr int64_t kTargetWgs = 512;  // ~2 workgroups per CU over 256 CUs

__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// o[s] = row[h * KH + s] (global or LDS)
template <int KH>
__device__ __forceinline__ void ld_half(float (&o)[KH], const float* row, int h) {
  const float4* p = reinterpret_cast<const float4*>(row + h * KH);
#pragma unroll
  for (int q = 0; q < KH / 4; ++q) {
    const float4 t = p[q];
    o[4 * q] = t.x; o[4 * q + 1] = t.y; o[4 * q + 2] = t.z; o[4 * q + 3] = t.w;
  }
}

// ---- the streamed operand: 32-row tiles through double-buffered LDS ---------------
// The workgroup's 4 waves own 128 fixed rows (one 32-row register operand
// each) and walk the same streamed tiles, so a tile is fetched from L2 once
// per workgroup.  Tiles move global -> LDS by LDS-DMA (global_load_lds,
// 16 B per lane), issued for tile t+1 before tile t is consumed.  The DMA
// image is lane-linear (rows of D floats back to back), so the bank spread
// comes from an XOR swizzle applied on the global side: physical 16-B slot
// `p` of row r holds logical slot p ^ (r mod D/4).  A lane reading 16 B of
// row j at logical slot c reads physical slot c ^ (j mod D/4): the 16 rows
// of a read phase land in 16 distinct bank groups.
template <int D>
struct Stream {
  static constexpr int NS = D / 4;                // 16-B slots per row
  static constexpr int NI = kTile * D * 4 / 1024; // 1-KB wave DMA instructions per tile
  static constexpr int FLOATS = kTile * D;
};

template <int D>
__device__ __forceinline__ void tile_dma(float* buf, const float* M, int64_t r0, int64_t n) {
  using S = Stream<D>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i0 = 0; i0 < S::NI; i0 += kWaves) {
    const int i = i0 + wave;
    if (S::NI % kWaves == 0 || i < S::NI) {
      const int p = i * 64 + lane;
      const int row = p / S::NS, slot = p % S::NS;
      const float* g = M + min(r0 + row, n - 1) * D + (slot ^ (row % S::NS)) * 4;
      __builtin_amdgcn_global_load_lds(g, (lds_ptr_t)(buf + i * 256), 16, 0, 0);
    }
  }
}

// per-row lse (f32) and target (i64) of rows [r0, r0 + 32) -> LDS (wave 0)
__device__ __forceinline__ void rowdata_dma(float* lbuf, int64_t* tbuf, const float* lse,
                                            const int64_t* tgt, int64_t r0, int64_t n) {
  const int lane = threadIdx.x & 63;
  if ((threadIdx.x >> 6) != 0) return;
  __builtin_amdgcn_global_load_lds(lse + min(r0 + (lane & 31), n - 1), (lds_ptr_t)lbuf, 4, 0, 0);
  const char* tp = reinterpret_cast<const char*>(tgt + min(r0 + (lane >> 1), n - 1)) + (lane & 1) * 4;
  __builtin_amdgcn_global_load_lds(tp, (lds_ptr_t)tbuf, 4, 0, 0);
}

// per-row int32 exponents of rows [r0, r0 + 32) -> LDS (wave 0; lanes 32-63
// repeat them into the buffer's upper half)
__device__ __forceinline__ void rowexp_dma(float* ebuf, const float* ex, int64_t r0, int64_t n) {
  const int lane = threadIdx.x & 63;
  if ((threadIdx.x >> 6) != 0) return;
  __builtin_amdgcn_global_load_lds(ex + min(r0 + (lane & 31), n - 1), (lds_ptr_t)ebuf, 4, 0, 0);
}

template <int D>
__device__ __forceinline__ float lds_at(const float* tile, int row, int col) {
  using S = Stream<D>;
  return tile[row * D + (((col >> 2) ^ (row % S::NS)) << 2) + (col & 3)];
}

// Operand reads of the second GEMM: element [crow(s, h)][n*32 + j] of a
// swizzled tile.  With row = R_s + 4h (R_s = (s&3) + 8(s>>2), bit 2 clear)
// the swizzle splits into a lane part that depends only on s&3 and a
// compile-time part, so each read is one ds_read_b32 with an immediate
// offset from one of four per-lane bases.  D >= 32.
template <int D>
struct ColReader {
  int base[4];
  __device__ __forceinline__ ColReader(int j, int h) {
    constexpr int NS = Stream<D>::NS;
    const int H = NS > 4 ? 4 * h : 0;
    const int Lh = (j >> 2) ^ H;
#pragma unroll
    for (int q = 0; q < 4; ++q) base[q] = 4 * h * D + (j & 3) + ((Lh ^ q) << 2);
  }
  template <int S_, int N_>
  __device__ __forceinline__ float at(const float* tile) const {
    constexpr int NS = Stream<D>::NS;
    constexpr int R = (S_ & 3) + 8 * (S_ >> 2);
    constexpr int Xc = R % NS;
    constexpr int off = R * D + (((N_ * 8) ^ (Xc & ~7)) << 2);
    return tile[base[S_ & 3] + off];
  }
};

// X = A B over the full depth with one operand's row j read from a swizzled
// LDS tile (kTileIsA: the tile supplies A) and the other held in registers.
// The tile reads run two 16-B loads ahead of the MFMAs consuming them.
template <int D, int KH, bool kTileIsA>
__device__ __forceinline__ f32x16 lds_dot(const float* tile, int j, int h, const float (&r)[KH]) {
  constexpr int NQ = KH / 4;
  constexpr int AHEAD = NQ < 2 ? NQ : 2;
  const float* row = tile + j * D;
  int sw = j % Stream<D>::NS;
  // opaque per call: keeps the 16 swizzled addresses out of loop-invariant
  // code motion (hoisted, they would pin 16-32 VGPRs for the whole loop)
  asm volatile("" : "+v"(sw));
  auto rd = [&](int q) {
    return *reinterpret_cast<const float4*>(row + (((h * KH / 4) + q) ^ sw) * 4);
  };
  float4 w[NQ];
#pragma unroll
  for (int q = 0; q < AHEAD; ++q) w[q] = rd(q);
  f32x16 acc = {};
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    if (q + AHEAD < NQ) w[q + AHEAD] = rd(q + AHEAD);
    __builtin_amdgcn_sched_barrier(0);
    const float t[4] = {w[q].x, w[q].y, w[q].z, w[q].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = kTileIsA ? t[e] : r[4 * q + e];
      const float b = kTileIsA ? r[4 * q + e] : t[e];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// acc[n] += P^T-operand (registers p, the accumulator tile of the first
// GEMM) x tile rows crow(s, h), columns n*32 + j: the second GEMM of the CE
// backward.  The NT accumulator chains are interleaved.
template <int D, int NT>
__device__ __forceinline__ void gemm2(f32x16 (&acc)[NT], const float (&p)[16], const float* tile,
                                      const ColReader<D>& cr, int j, int h) {
  if constexpr (D >= 32) {
    static_for<0, 16>([&](auto s) {
      static_for<0, NT>([&](auto n) {
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[s], cr.template at<s, n>(tile), acc[n], 0,
                                                      0, 0);
      });
    });
  } else {
    const int col = min(j, D - 1);
#pragma unroll
    for (int s = 0; s < 16; ++s)
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[s], lds_at<D>(tile, crow(s, h), col), acc[0],
                                                    0, 0, 0);
  }
}

// Tile-relative bounds for the epilogues: item/row index v0 + c is valid when
// lo <= c < hi, and is the target when c == tt (all int32, branch-free).
__device__ __forceinline__ int rel32(int64_t x, int64_t v0) {
  return (int)max<int64_t>(-1, min<int64_t>(x - v0, kTile + 1));
}

// log-sum-exp state (m, s): sum_i exp(x_i) = s * exp(m)
__device__ __forceinline__ void lse_push(float& m, float& s, float x) {
  const float d = x - m;
  const float e = fexp(-fabsf(d));
  s = d > 0.0f ? fmaf(s, e, 1.0f) : s + e;
  m = fmaxf(m, x);
}
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;
  s = s * fexp(m - M) + s2 * fexp(m2 - M);
  m = M;
}

// ---- allow-bitmaps: a filter is one 32-bit word per 32-item tile --------------------
// AllowArgs (common.h): words [F, W] int32, rows [B] int64 or null.
//
// One row's view of its filter.  rows null: filter 0.  f == -1: every item is
// allowed; f outside [-1, F): none is.  The filter and word indices are
// clamped for the load and the loaded word masked, so nothing is ever read out
// of range.
struct AllowRow {
  const int* w;
  int64_t last;
  unsigned keep, force;   // the row's word = (loaded & keep) | force
  __device__ __forceinline__ AllowRow(const AllowArgs& a, int64_t b) {
    const int64_t f = a.rows ? a.rows[b] : 0;
    w = a.words + max<int64_t>(0, min<int64_t>(f, a.F - 1)) * a.W;
    last = a.W - 1;
    keep = (f >= 0 && f < a.F) ? ~0u : 0u;
    force = f == -1 ? ~0u : 0u;
  }
  __device__ __forceinline__ unsigned word(int64_t t) const {
    return ((unsigned)w[max<int64_t>(0, min<int64_t>(t, last))] & keep) | force;
  }
  // every item allowed, for a kAllow kernel called without a filter; `any`
  // is readable memory of at least one word (its value is masked away)
  __device__ __forceinline__ static AllowRow all(const void* any) {
    AllowRow r;
    r.w = static_cast<const int*>(any);
    r.last = 0;
    r.keep = 0u;
    r.force = ~0u;
    return r;
  }

 private:
  AllowRow() = default;
};

// bit r of the result = bit crow(r, h) of a tile's word: a lane's 16 items
__device__ __forceinline__ unsigned lane_bits(unsigned a, int h) {
  a >>= 4 * h;
  return (a & 0xfu) | ((a >> 4) & 0xf0u) | ((a >> 8) & 0xf00u) | ((a >> 12) & 0xf000u);
}

// ---- score priors: a per-item term, weighted per row (include/recblr_priors.h) -----
// PriorArgs (common.h): values [P, V] fp32, rows [B] int64 or null, weight [B]
// fp32 or null.
//
// One row's view of its prior.  rows null: prior 0.  f == -1: the row takes no
// prior (its scores stay as they are, bit for bit); f outside [-1, P): the row
// selects nothing.  The prior and item indices are clamped for the load and the
// loaded value is used only where `on`, so nothing is ever read out of range.
struct PriorRow {
  const float* p = nullptr;
  int64_t idx = 0, last = 0;   // the clamped prior index; V - 1
  float w = 0.0f;
  bool on = false, none = false;
  PriorRow() = default;
  __device__ __forceinline__ PriorRow(const PriorArgs& a, int64_t b) {
    const int64_t f = a.rows ? a.rows[b] : 0;
    idx = max<int64_t>(0, min<int64_t>(f, a.P - 1));
    p = a.values + idx * a.V;
    last = a.V - 1;
    w = a.weight ? a.weight[b] : 1.0f;
    on = f >= 0 && f < a.P;
    none = f < -1 || f >= a.P;
  }
  __device__ __forceinline__ float at(int64_t v) const {
    return p[max<int64_t>(0, min<int64_t>(v, last))];
  }
  // score + (w * prior): the product rounded, then the sum (no fma); a select,
  // not an addition of zero, where the row takes no prior
  __device__ __forceinline__ float adj(float s, float pv) const {
    return on ? __fadd_rn(s, __fmul_rn(w, pv)) : s;
  }
};

// The prior over a lane's walk of the item tiles: the lane owns one sequence and
// the 16 items crow(r, h) of a tile, so it needs 16 values of its row's prior
// per tile.  Where the wave's 32 sequences take one prior row (the common case;
// a sequence without a prior counts as taking row 0) the tile's 32 values are
// read one per lane, one tile ahead, and fetched by shuffle; otherwise each
// lane gathers its own 16 ahead of the tile's MFMA chain.  The choice is a
// ballot taken once, so it is wave-uniform.  kPrior false: nothing.
template <bool kPrior>
struct PriorSweep {
  PriorRow pr;
  bool shared = false;
  float pw = 0.0f;    // the next tile's value of item 32 t + j (shared)
  float pv[16] = {};  // this tile's values of the lane's items
  __device__ __forceinline__ PriorSweep(const PriorArgs& pa, int64_t b, int64_t t0, int j) {
    if constexpr (kPrior) {
      pr = PriorRow(pa, b);
      shared = __builtin_amdgcn_ballot_w64(pr.idx != __shfl(pr.idx, 0)) == 0;
      if (shared) pw = pr.at(t0 * kTile + j);
    }
  }
  // before tile t's MFMA chain: the loads
  __device__ __forceinline__ void load(int64_t t, int j, int h) {
    if constexpr (kPrior) {
      if (shared) {
        pv[0] = pw;
        pw = pr.at((t + 1) * kTile + j);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) pv[r] = pr.at(t * kTile + crow(r, h));
      }
    }
  }
  // after it: the tile's scores become the adjusted scores
  __device__ __forceinline__ void apply(f32x16& x, int h) {
    if constexpr (kPrior) {
      if (shared) {
        const float pt = pv[0];
#pragma unroll
        for (int r = 0; r < 16; ++r) pv[r] = __shfl(pt, crow(r, h));
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) x[r] = pr.adj(x[r], pv[r]);
    }
  }
};

// ---- target scores: the MFMA chain order, one thread per row ------------------
// kAllow: a target its row's filter does not allow counts as out of range (al
// without words, in a kPrior kernel: no filter).  kPrior: the target's score
// is adjusted by its row's prior; a row whose prior index selects nothing, like
// a NaN adjusted score, counts as out of range.
template <int D, bool kAllow, bool kPrior = false>
__device__ __forceinline__ void target_dot(const float* __restrict__ E,
                                           const float* __restrict__ W,
                                           const int64_t* __restrict__ tgt, int64_t B, int64_t V,
                                           float* __restrict__ ts, const AllowArgs& al,
                                           const PriorArgs& pa = PriorArgs{}) {
  constexpr int KH = D / 2;
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int64_t t = tgt[b];
  if (t < 0 || t >= V) {
    ts[b] = NAN;
    return;
  }
  if constexpr (kAllow) {
    if (!kPrior || al.words) {
      if (!((AllowRow(al, b).word(t >> 5) >> (t & 31)) & 1u)) {
        ts[b] = NAN;
        return;
      }
    }
  }
  PriorRow pr;
  if constexpr (kPrior) {
    pr = PriorRow(pa, b);
    if (pr.none) {
      ts[b] = NAN;
      return;
    }
  }
  float e0[KH], e1[KH], w0[KH], w1[KH];
  ld_half<KH>(e0, E + b * D, 0);
  ld_half<KH>(e1, E + b * D, 1);
  ld_half<KH>(w0, W + t * D, 0);
  ld_half<KH>(w1, W + t * D, 1);
  float acc = 0.0f;
#pragma unroll
  for (int s = 0; s < KH; ++s) {
    acc = fmaf(w0[s], e0[s], acc);
    acc = fmaf(w1[s], e1[s], acc);
  }
  if constexpr (kPrior) acc = pr.adj(acc, pr.at(t));
  ts[b] = acc;
}

template <int D>
__global__ __launch_bounds__(256) void k_target_dot(const float* __restrict__ E,
                                                    const float* __restrict__ W,
                                                    const int64_t* __restrict__ tgt, int64_t B,
                                                    int64_t V, float* __restrict__ ts) {
  target_dot<D, false>(E, W, tgt, B, V, ts, AllowArgs{});
}

template <int D>
__global__ __launch_bounds__(256) void k_target_dot_allowed(const float* __restrict__ E,
                                                            const float* __restrict__ W,
                                                            const int64_t* __restrict__ tgt,
                                                            int64_t B, int64_t V,
                                                            float* __restrict__ ts, AllowArgs al) {
  target_dot<D, true>(E, W, tgt, B, V, ts, al);
}

template <int D>
__global__ __launch_bounds__(256) void k_target_dot_prior(const float* __restrict__ E,
                                                          const float* __restrict__ W,
                                                          const int64_t* __restrict__ tgt,
                                                          int64_t B, int64_t V,
                                                          float* __restrict__ ts, AllowArgs al,
                                                          PriorArgs pa) {
  target_dot<D, true, true>(E, W, tgt, B, V, ts, al, pa);
}

// Workgroup placement.  The grid is 1-D over RB fixed-row blocks x S splits
// of the streamed operand (S padded to a multiple of 8).  Workgroups are
// dealt to the 8 XCDs round-robin by linear id, so giving split s only ids
// with id % 8 == s % 8 keeps every slice of the streamed operand in one
// XCD's L2 (each XCD streams 1/8 of it) instead of all eight.
struct Place {
  int64_t rb, split;
};

__device__ __forceinline__ bool place(int64_t RB, int64_t S, Place& p) {
  const int64_t L = blockIdx.x, xcd = L & 7, k = L >> 3;
  p.rb = k % RB;
  p.split = (k / RB) * 8 + xcd;
  return p.split < S;
}

// Shared frame of the row-stationary kernels: the workgroup's 4 waves own
// 128 fixed rows (32 per wave) and walk tiles [split*per, ...) of `strm`
// [n_strm, D].  body(tile_index, lds_tile, lds_lse, lds_tgt) runs once per
// streamed tile with the tile resident in LDS; with kRowData 1 the tile's
// per-row lse / target values ride along, with 2 the per-row int32 scale
// exponents of a split image (passed as lse_g, landing in lds_lse), with 3
// all three (the exponents from ex_g into a fifth body argument).
template <int D, int kRowData, class Body>
__device__ __forceinline__ void stream_tiles(const float* strm, int64_t n_strm, int64_t per,
                                             int64_t split, const float* lse_g,
                                             const int64_t* tgt_g, Body&& body,
                                             const float* ex_g = nullptr) {
  using S = Stream<D>;
  // two distinct LDS objects (not one indexed array): the compiler then sees
  // that reads of one buffer cannot alias the DMA in flight into the other
  // and does not drain the DMA (vmcnt(0)) before them
  __shared__ __attribute__((aligned(16))) float buf0[S::FLOATS];
  __shared__ __attribute__((aligned(16))) float buf1[S::FLOATS];
  __shared__ __attribute__((aligned(16))) float lbuf0[64];
  __shared__ __attribute__((aligned(16))) float lbuf1[64];
  __shared__ __attribute__((aligned(16))) int64_t tbuf0[32];
  __shared__ __attribute__((aligned(16))) int64_t tbuf1[32];
  __shared__ __attribute__((aligned(16))) float xbuf0[kRowData == 3 ? 64 : 1];
  __shared__ __attribute__((aligned(16))) float xbuf1[kRowData == 3 ? 64 : 1];
  const int64_t nt = (n_strm + kTile - 1) / kTile;
  const int64_t t0 = split * per, t1 = min(t0 + per, nt);
  if (t0 >= t1) return;
  auto issue = [&](int64_t t, float* b, float* lb, int64_t* tb, float* xb) {
    tile_dma<D>(b, strm, t * kTile, n_strm);
    if constexpr (kRowData == 1 || kRowData == 3) rowdata_dma(lb, tb, lse_g, tgt_g, t * kTile, n_strm);
    if constexpr (kRowData == 2) rowexp_dma(lb, lse_g, t * kTile, n_strm);
    if constexpr (kRowData == 3) rowexp_dma(xb, ex_g, t * kTile, n_strm);
  };
  auto run = [&](int64_t t, const float* b, const float* lb, const int64_t* tb, const float* xb) {
    if constexpr (kRowData == 3) body(t, b, lb, tb, xb);
    else body(t, b, lb, tb);
  };
  issue(t0, buf0, lbuf0, tbuf0, xbuf0);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  for (int64_t t = t0; t < t1; t += 2) {
    if (t + 1 < t1) issue(t + 1, buf1, lbuf1, tbuf1, xbuf1);
    run(t, buf0, lbuf0, tbuf0, xbuf0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (t + 1 >= t1) break;
    if (t + 2 < t1) issue(t + 2, buf0, lbuf0, tbuf0, xbuf0);
    run(t + 1, buf1, lbuf1, tbuf1, xbuf1);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
  }
}

// ---- CE forward: per (row, vocab split) log-sum-exp partials --------------------
// Tile orientation X^T[v][b] (A = item rows from LDS, B = sequence rows in
// registers): each lane holds one sequence row b and 16 items per tile, so
// its running (m, s) is one pair; the two lane halves merge at the end.  The
// lane whose tile holds b's target stores that score (bit-identical to the
// value inside the log-sum-exp).
template <int D>
__global__ __launch_bounds__(256) void k_ce_fwd(const float* __restrict__ E,
                                                const float* __restrict__ W,
                                                const int64_t* __restrict__ tgt, int64_t B,
                                                int64_t V, int64_t per, int64_t RB, int64_t NS, float* __restrict__ m_part,
                                                float* __restrict__ s_part,
                                                float* __restrict__ ts,
                                                unsigned* __restrict__ ticket) {
  constexpr int KH = D / 2;
  if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b = (pl.rb * kWaves + wave) * kTile + j;
  const int64_t bc = min(b, B - 1);
  float eb[KH];
  ld_half<KH>(eb, E + bc * D, h);
  const int64_t tb = tgt[bc];
  float m = -INFINITY, s = 0.0f, tsv = 0.0f;
  bool has_ts = false;
  stream_tiles<D, false>(W, V, per, pl.split, nullptr, nullptr,
                         [&](int64_t t, const float* tile, const float*, const int64_t*) {
    const int64_t v0 = t * kTile;
    const f32x16 x = lds_dot<D, KH, true>(tile, j, h, eb);
    const int hi = rel32(V, v0), tt = rel32(tb, v0);
    if (hi >= kTile) {
#pragma unroll
      for (int r = 0; r < 16; ++r) lse_push(m, s, x[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (crow(r, h) < hi) lse_push(m, s, x[r]);
    }
    if (tt >= 0 && tt < kTile) {   // this tile holds the row's target
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (crow(r, h) == tt) {
          tsv = x[r];
          has_ts = true;
        }
    }
  });
  if (has_ts && b < B) ts[b] = tsv;
  lse_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
  if (h == 0 && b < B) {
    m_part[pl.split * B + b] = m;
    s_part[pl.split * B + b] = s;
  }
}

// lse[b] over the S splits (a lane per row, four waves over the splits), the
// per-row loss lse - score(target) (NaN for an out-of-range target, which
// k_ce_fwd never matches), and - in the workgroup that finishes last - the
// batch mean in a fixed order.  `ticket` is zeroed by k_ce_fwd.
// ROWS (the row-chunked CE with ignorable rows, rb_item_ce_fwd_h_rows): a
// target of -1 is an ignored row (loss 0, lse still written), and loss[0] is
// the sum of the rows' losses times the caller's inv_n, added to what loss[0]
// holds when `accumulate` (the chunks of one call run in stream order).
template <bool ROWS>
__global__ __launch_bounds__(256) void k_ce_rows(const float* __restrict__ m_part,
                                                 const float* __restrict__ s_part, int64_t S,
                                                 const float* __restrict__ ts,
                                                 const int64_t* __restrict__ tgt, int64_t B,
                                                 int64_t V, float* __restrict__ lse,
                                                 float* __restrict__ loss_rows,
                                                 unsigned* __restrict__ ticket,
                                                 float* __restrict__ loss, float inv_n,
                                                 int accumulate) {
  // 64 rows per workgroup, one per lane; wave w merges splits w, w + 4, ...
  // in order (coalesced: a wave reads 64 consecutive rows of a split), then
  // the four waves' states merge in wave order
  __shared__ float red[256];
  __shared__ float sm[4][64], ss[4][64];
  __shared__ bool last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t b = (int64_t)blockIdx.x * 64 + lane;
  const int64_t bc = b < B ? b : B - 1;
  float m = -INFINITY, s = 0.0f;
  for (int64_t i = w; i < S; i += 4) lse_merge(m, s, m_part[i * B + bc], s_part[i * B + bc]);
  sm[w][lane] = m;
  ss[w][lane] = s;
  __syncthreads();
  if (w == 0 && b < B) {
#pragma unroll
    for (int k = 1; k < 4; ++k) lse_merge(m, s, sm[k][lane], ss[k][lane]);
    const float l = m + logf(s);
    const int64_t t = tgt[b];
    lse[b] = l;
    loss_rows[b] = (ROWS && t == -1) ? 0.0f : (t < 0 || t >= V) ? NAN : l - ts[b];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float acc = 0.0f;
  for (int64_t i = threadIdx.x; i < B; i += 256) acc += loss_rows[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if constexpr (ROWS) loss[0] = (accumulate ? loss[0] : 0.0f) + red[0] * inv_n;
    else loss[0] = red[0] / (float)B;
    *ticket = 0u;
  }
}

// ---- CE backward, dE = P W (per vocab split partials) ----------------------------
// P[b][v] = (exp(x - lse[b]) - [v == target[b]]) * dloss / B
template <int D>
__global__ __launch_bounds__(256) void k_ce_bwd_seq(const float* __restrict__ E,
                                                    const float* __restrict__ W,
                                                    const float* __restrict__ lse,
                                                    const int64_t* __restrict__ tgt,
                                                    const float* __restrict__ dloss, float inv_n,
                                                    int64_t B, int64_t V, int64_t per, int64_t RB, int64_t NS,
                                                    float* __restrict__ de_part) {
  constexpr int KH = D / 2, NT = (D + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b0 = (pl.rb * kWaves + wave) * kTile;
  const int64_t b = min(b0 + j, B - 1);
  float eb[KH];
  ld_half<KH>(eb, E + b * D, h);
  const float lb = lse[b];
  const int64_t tb = tgt[b];
  const float g = dloss[0] * inv_n;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x16{};
  const ColReader<D> cr(j, h);
  stream_tiles<D, false>(W, V, per, pl.split, nullptr, nullptr,
                         [&](int64_t t, const float* tile, const float*, const int64_t*) {
    const int64_t v0 = t * kTile;
    const f32x16 x = lds_dot<D, KH, true>(tile, j, h, eb);
    const int hi = rel32(V, v0), tt = rel32(tb, v0);
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = crow(r, h);
      const float sm = fexp(x[r] - lb) - (c == tt ? 1.0f : 0.0f);
      p[r] = c < hi ? sm * g : 0.0f;
    }
    gemm2<D, NT>(acc, p, tile, cr, j, h);
  });
  if (b0 >= B) return;
  float* out = de_part + pl.split * B * D;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = n * 32 + j;
    if (col >= D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = b0 + crow(r, h);
      if (row < B) out[row * D + col] = acc[n][r];
    }
  }
}

// ---- CE backward, dW = P^T E (per row split partials) ----------------------------
// Tile orientation X[b][v] (A = sequence rows from LDS, B = item rows in
// registers): lane holds item column v, so X is the A operand of P^T E.
template <int D>
__global__ __launch_bounds__(256) void k_ce_bwd_item(const float* __restrict__ E,
                                                     const float* __restrict__ W,
                                                     const float* __restrict__ lse,
                                                     const int64_t* __restrict__ tgt,
                                                     const float* __restrict__ dloss, float inv_n,
                                                     int64_t B, int64_t V, int64_t per, int64_t RB, int64_t NS,
                                                     float* __restrict__ dw_part) {
  constexpr int KH = D / 2, NT = (D + 31) / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t v0 = (pl.rb * kWaves + wave) * kTile;
  const int64_t v = v0 + j;
  float wb[KH];
  ld_half<KH>(wb, W + min(v, V - 1) * D, h);
  const float g = dloss[0] * inv_n;
  f32x16 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x16{};
  const ColReader<D> cr(j, h);
  stream_tiles<D, true>(E, B, per, pl.split, lse, tgt,
                        [&](int64_t t, const float* tile, const float* lt, const int64_t* tt) {
    const int64_t b0 = t * kTile;
    const f32x16 x = lds_dot<D, KH, true>(tile, j, h, wb);
    const int hi = rel32(B, b0);
    float p[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = crow(r, h);
      const float sm = fexp(x[r] - lt[c]) - (v == tt[c] ? 1.0f : 0.0f);
      p[r] = c < hi ? sm * g : 0.0f;
    }
    gemm2<D, NT>(acc, p, tile, cr, j, h);
  });
  if (v0 >= V) return;
  float* out = dw_part + pl.split * V * D;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int col = n * 32 + j;
    if (col >= D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = v0 + crow(r, h);
      if (row < V) out[row * D + col] = acc[n][r];
    }
  }
}

// out[i] = sum_p parts[p * n + i], p in order
__global__ __launch_bounds__(256) void k_sum_parts(const float* __restrict__ parts, int64_t P,
                                                   int64_t n, float* __restrict__ out) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (i4 + 4 <= n && (n & 3) == 0) {
    float4 acc = *reinterpret_cast<const float4*>(parts + i4);
    for (int64_t p = 1; p < P; ++p) {
      const float4 t = *reinterpret_cast<const float4*>(parts + p * n + i4);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    *reinterpret_cast<float4*>(out + i4) = acc;
  } else {
    for (int64_t i = i4; i < min(i4 + 4, n); ++i) {
      float acc = parts[i];
      for (int64_t p = 1; p < P; ++p) acc += parts[p * n + i];
      out[i] = acc;
    }
  }
}

// ---- ranks: #items scoring above / equal to the target -----------------------------
// kAllow: only items that the row's filter allows are counted; tile t of the
// items is word t of the filter, read one tile ahead of its use.
// kPrior: the counts run over the adjusted scores (ts holds the target's).
template <int D, bool kAllow, bool kPrior = false>
__device__ __forceinline__ void item_rank(const float* __restrict__ E,
                                          const float* __restrict__ W,
                                          const float* __restrict__ ts,
                                          const int64_t* __restrict__ tgt, int64_t B, int64_t V,
                                          int64_t first, int64_t per, int64_t RB, int64_t NS,
                                          int* __restrict__ gt_part, int* __restrict__ eq_part,
                                          const AllowArgs& al,
                                          const PriorArgs& pa = PriorArgs{}) {
  constexpr int KH = D / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b = (pl.rb * kWaves + wave) * kTile + j;
  const int64_t bc = min(b, B - 1);
  float eb[KH];
  ld_half<KH>(eb, E + bc * D, h);
  const float tsb = ts[bc];
  const int64_t tb = tgt[bc];
  int gt = 0, eq = 0;
  const AllowRow ar(al, kAllow ? bc : 0);
  unsigned aw = kAllow ? ar.word(pl.split * per) : 0u;   // the next tile's word
  PriorSweep<kPrior> ps(pa, bc, pl.split * per, j);
  stream_tiles<D, false>(W, V, per, pl.split, nullptr, nullptr,
                         [&](int64_t t, const float* tile, const float*, const int64_t*) {
    const int64_t v0 = t * kTile;
    unsigned am = 0xffffu;
    if constexpr (kAllow) {
      am = lane_bits(aw, h);
      aw = ar.word(t + 1);
    }
    ps.load(t, j, h);
    f32x16 x = lds_dot<D, KH, true>(tile, j, h, eb);
    ps.apply(x, h);
    const int lo = rel32(first, v0), hi = rel32(V, v0), tt = rel32(tb, v0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = crow(r, h);
      bool ok = (c >= lo) & (c < hi) & (c != tt);
      if constexpr (kAllow) ok &= (am >> r) & 1u;
      gt += (ok & (x[r] > tsb)) ? 1 : 0;
      eq += (ok & (x[r] == tsb)) ? 1 : 0;
    }
  });
  gt += __shfl_xor(gt, 32);
  eq += __shfl_xor(eq, 32);
  if (h == 0 && b < B) {
    gt_part[pl.split * B + b] = gt;
    eq_part[pl.split * B + b] = eq;
  }
}

template <int D>
__global__ __launch_bounds__(256) void k_item_rank(const float* __restrict__ E,
                                                   const float* __restrict__ W,
                                                   const float* __restrict__ ts,
                                                   const int64_t* __restrict__ tgt, int64_t B,
                                                   int64_t V, int64_t first, int64_t per, int64_t RB, int64_t NS,
                                                   int* __restrict__ gt_part,
                                                   int* __restrict__ eq_part) {
  item_rank<D, false>(E, W, ts, tgt, B, V, first, per, RB, NS, gt_part, eq_part, AllowArgs{});
}

template <int D>
__global__ __launch_bounds__(256) void k_item_rank_allowed(
    const float* __restrict__ E, const float* __restrict__ W, const float* __restrict__ ts,
    const int64_t* __restrict__ tgt, int64_t B, int64_t V, int64_t first, int64_t per, int64_t RB,
    int64_t NS, int* __restrict__ gt_part, int* __restrict__ eq_part, AllowArgs al) {
  item_rank<D, true>(E, W, ts, tgt, B, V, first, per, RB, NS, gt_part, eq_part, al);
}

template <int D, bool kAllow>
__global__ __launch_bounds__(256) void k_item_rank_prior(
    const float* __restrict__ E, const float* __restrict__ W, const float* __restrict__ ts,
    const int64_t* __restrict__ tgt, int64_t B, int64_t V, int64_t first, int64_t per, int64_t RB,
    int64_t NS, int* __restrict__ gt_part, int* __restrict__ eq_part, AllowArgs al, PriorArgs pa) {
  item_rank<D, kAllow, true>(E, W, ts, tgt, B, V, first, per, RB, NS, gt_part, eq_part, al, pa);
}

__global__ __launch_bounds__(256) void k_rank_rows(const int* __restrict__ gt_part,
                                                   const int* __restrict__ eq_part, int64_t S,
                                                   const float* __restrict__ ts, int64_t B,
                                                   int64_t* __restrict__ n_gt,
                                                   int64_t* __restrict__ n_eq) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int64_t g = 0, e = 0;
  for (int64_t i = 0; i < S; ++i) {
    g += gt_part[i * B + b];
    e += eq_part[i * B + b];
  }
  const bool bad = ts[b] != ts[b];  // NaN: target id out of range
  n_gt[b] = bad ? -1 : g;
  if (n_eq) n_eq[b] = bad ? -1 : e;
}

// ---- top-k: each row's k best items, no score matrix -------------------------------
// k_item_rank's frame (a lane owns sequence row b and sees 16 items per
// tile) with a selection epilogue.  Candidates order by (score descending,
// id ascending): `beats` below.  Per (row, split) a list of k candidates
// lives in LDS, unsorted, owned by the row's h = 0 lane, which keeps the
// list's worst entry (score, id, position) in registers as the admission
// threshold.  A score passes the cheap filter when it is >= the threshold
// score (false for NaN); the h = 1 lane hands its passing candidates to h = 0
// by shuffle, so one lane writes a list.  An admitted candidate replaces the
// worst entry and the list is rescanned for the new worst (k independent LDS
// reads, no dependent shift chain).  Empty slots are (-inf, kNoItem), which
// every real candidate beats, a -inf score included.
//
// Exclusion: the row's two lanes hash the exclude entries that fall into the
// split's item range into the row's kExBits-bit map in LDS (atomic OR: the
// map does not depend on the order).  A candidate whose bit is clear is not
// excluded; a set bit is confirmed by scanning the row's list unless the
// split's range fits the map (then the map is exact: the evaluation shape's
// 352-item splits).  Only candidates that beat the threshold pay for the
// lookup.
constexpr int kNoItem = 0x7fffffff;
constexpr int kExBits = 512;   // exclusion map bits per row

__device__ __forceinline__ bool beats(float s, int id, float s2, int id2) {
  return s > s2 || (s == s2 && id < id2);
}

// kAllow: tile t of the items is word t of the row's filter, so the filter is
// one AND into the pass mask per tile, ahead of the admission loop: an item the
// filter drops is never a candidate, and a sparse filter shortens the loop.
// The word is read one tile ahead of its use.
//
// kGroup (include/recblr_groups.h): at most gr.m entries of one group in a
// list.  Every entry carries its group (16 bits in LDS, kNoGroup for an
// uncapped item and for an empty slot), and the list stays the k best of U =
// each group's m best items seen so far plus every uncapped item.  A candidate
// that passes the threshold and whose group already holds m entries replaces
// that group's worst entry if it beats it (also while the list has empty
// slots), else it is dropped; any other candidate replaces the list's worst as
// before.  The group's count and worst come from one scan of the k entries.
// Replacing an entry that is not the list's worst leaves the threshold as it
// is (the newcomer beats an entry that the worst does not beat), so only a
// replaced worst is followed by the rescan.  A tile's 32 group ids are read
// one per lane, one tile ahead, and a candidate's id is fetched by shuffle.
// GroupArgs: common.h.
constexpr int kNoGroup = 0xffff;

//
// kPrior (include/recblr_priors.h): a tile's scores become the adjusted scores
// right after the MFMA chain (PriorSweep), ahead of the threshold compare, so
// the filter, the exclusion, the cap, the lists and the merge over the splits
// see adjusted scores and nothing else changes; a row whose prior index selects
// nothing passes no score.  al without words (a kAllow kernel called without a
// filter): every item allowed.  No LDS of its own.
template <int D, int KP, bool kAllow, bool kGroup = false, bool kPrior = false>
__device__ __forceinline__ void item_topk(const float* __restrict__ E,
                                          const float* __restrict__ W, int64_t B, int64_t V,
                                          int64_t first, int k, const int64_t* __restrict__ ex,
                                          int64_t NE, int64_t per, int64_t RB, int64_t NS,
                                          float* __restrict__ c_sc, int* __restrict__ c_id,
                                          float* l_sc, int* l_id, unsigned* l_ex,
                                          const AllowArgs& al, int* __restrict__ c_g = nullptr,
                                          unsigned short* l_g = nullptr,
                                          const GroupArgs& gr = GroupArgs{},
                                          const PriorArgs& pa = PriorArgs{}) {
  constexpr int KH = D / 2, NR = kWaves * kTile, XW = kExBits / 32;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b = (pl.rb * kWaves + wave) * kTile + j;
  const int64_t bc = min(b, B - 1);
  float eb[KH];
  ld_half<KH>(eb, E + bc * D, h);
  const int row = wave * kTile + j;
  // the split's item range [v_lo, v_hi)
  const int64_t v_lo = pl.split * per * kTile, v_hi = min((pl.split + 1) * per * kTile, V);
  const bool ex_exact = v_hi - v_lo <= kExBits;
  const int64_t* exr = ex + bc * NE;
  if (h == 0) {
    for (int i = 0; i < k; ++i) {
      l_sc[i * NR + row] = -INFINITY;
      l_id[i * NR + row] = kNoItem;
      if constexpr (kGroup) l_g[i * NR + row] = kNoGroup;
    }
  }
  if (NE > 0) {
#pragma unroll
    for (int w = 0; w < XW / 2; ++w) l_ex[(h * (XW / 2) + w) * NR + row] = 0u;
    __syncthreads();
    for (int64_t e = h; e < NE; e += 2) {
      const int64_t v = exr[e];
      if (v >= v_lo && v < v_hi) {
        const int hb = (int)(v - v_lo) & (kExBits - 1);
        atomicOr(&l_ex[(hb >> 5) * NR + row], 1u << (hb & 31));
      }
    }
  }
  __syncthreads();
  float thr = -INFINITY;   // the list's worst entry (h = 0 owns it; h = 1 holds a copy of thr)
  int thr_id = kNoItem, thr_pos = 0;
  auto excluded = [&](int id) -> bool {
    const int hb = (id - (int)v_lo) & (kExBits - 1);
    const unsigned wd = l_ex[(hb >> 5) * NR + row];
    if (!((wd >> (hb & 31)) & 1u)) return false;
    if (ex_exact) return true;
    for (int64_t e = 0; e < NE; ++e)
      if (exr[e] == (int64_t)id) return true;
    return false;
  };
  auto try_insert = [&](float s, int id, int g) {   // h = 0 lanes only
    if (!beats(s, id, thr, thr_id)) return;
    if (NE > 0 && excluded(id)) return;
    int pos = thr_pos;
    if constexpr (kGroup) {
      if (g != kNoGroup) {
        int cnt = 0, gi = 0;   // the group's entries and the worst of them
        float gs = 0.0f;
        for (int i = 0; i < k; ++i) {
          const float a = l_sc[i * NR + row];
          const int c = l_id[i * NR + row];
          if (l_g[i * NR + row] == g) {
            if (cnt == 0 || beats(gs, gi, a, c)) {
              gs = a;
              gi = c;
              pos = i;
            }
            ++cnt;
          }
        }
        if (cnt < gr.m) pos = thr_pos;
        else if (!beats(s, id, gs, gi)) return;
      }
      l_g[pos * NR + row] = (unsigned short)g;
    }
    l_sc[pos * NR + row] = s;
    l_id[pos * NR + row] = id;
    if constexpr (kGroup) {
      if (pos != thr_pos) return;
    }
    float ws = s;
    int wi = id, wp = thr_pos;
    for (int i = 0; i < k; ++i) {
      const float a = l_sc[i * NR + row];
      const int c = l_id[i * NR + row];
      if (beats(ws, wi, a, c)) {
        ws = a;
        wi = c;
        wp = i;
      }
    }
    thr = ws;
    thr_id = wi;
    thr_pos = wp;
  };
  const AllowRow ar = kPrior && kAllow && !al.words ? AllowRow::all(E)
                                                    : AllowRow(al, kAllow ? bc : 0);
  unsigned aw = kAllow ? ar.word(pl.split * per) : 0u;   // the next tile's word
  PriorSweep<kPrior> ps(pa, bc, pl.split * per, j);
  // group of item 32 t + j, clamped for the load (an item at or beyond V is no candidate)
  auto tile_group = [&](int64_t t) -> int {
    return gr.ids[max<int64_t>(0, min<int64_t>(t * kTile + j, V - 1))] & kNoGroup;
  };
  int gw = 0;   // the next tile's groups
  if constexpr (kGroup) gw = tile_group(pl.split * per);
  stream_tiles<D, false>(W, V, per, pl.split, nullptr, nullptr,
                         [&](int64_t t, const float* tile, const float*, const int64_t*) {
    const int64_t v0 = t * kTile;
    unsigned am = 0xffffu;
    if constexpr (kAllow) {
      am = lane_bits(aw, h);
      aw = ar.word(t + 1);
    }
    int gt = 0;
    if constexpr (kGroup) {
      gt = gw;
      gw = tile_group(t + 1);
    }
    ps.load(t, j, h);
    f32x16 x = lds_dot<D, KH, true>(tile, j, h, eb);
    ps.apply(x, h);
    const int lo = rel32(first, v0), hi = rel32(V, v0);
    unsigned m = 0;   // bit r: score r passes the cheap filter
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = crow(r, h);
      m |= ((c >= lo) & (c < hi) & (x[r] >= thr)) ? 1u << r : 0u;
    }
    if constexpr (kAllow) m &= am;
    if constexpr (kPrior) m = ps.pr.none ? 0u : m;
    // wave-uniform loop: every lane takes its lowest passing score per turn
    while (__builtin_amdgcn_ballot_w64(m != 0) != 0) {
      const bool p = m != 0;
      const int r = p ? __builtin_ctz(m) : 0;
      m &= m - 1;
      float cs = x[0];
#pragma unroll
      for (int q = 1; q < 16; ++q) cs = r == q ? x[q] : cs;
      const int cid = (int)v0 + crow(r, h);
      const float s1 = __shfl_xor(cs, 32);
      const int id1 = __shfl_xor(cid, 32);
      const int p1 = __shfl_xor((int)p, 32);
      int cg = 0, g1 = 0;
      if constexpr (kGroup) {
        cg = __shfl(gt, crow(r, h));
        g1 = __shfl_xor(cg, 32);
      }
      if (h == 0) {
        if (p) try_insert(cs, cid, cg);
        if (p1) try_insert(s1, id1, g1);
      }
      thr = __shfl(thr, j);
    }
  });
  if (h == 0 && b < B) {
    const int64_t o = (pl.split * B + b) * k;
    for (int i = 0; i < k; ++i) {
      c_sc[o + i] = l_sc[i * NR + row];
      c_id[o + i] = l_id[i * NR + row];
      if constexpr (kGroup) {
        const int g = l_g[i * NR + row];
        c_g[o + i] = g == kNoGroup ? -1 : g;
      }
    }
  }
}

// The kernels' LDS (the arrays belong to the kernel, not to item_topk: a kernel's
// LDS layout follows its own variables): entry i / map word w of row r at
// [i * NR + r] / [w * NR + r], so lanes of a wave touching the same entry or
// word hit distinct banks.
#define TOPK_LDS                                              \
  __shared__ float l_sc[KP * kWaves * kTile];                 \
  __shared__ int l_id[KP * kWaves * kTile];                   \
  __shared__ unsigned l_ex[kExBits / 32 * kWaves * kTile]

template <int D, int KP>
__global__ __launch_bounds__(256) void k_item_topk(const float* __restrict__ E,
                                                   const float* __restrict__ W, int64_t B,
                                                   int64_t V, int64_t first, int k,
                                                   const int64_t* __restrict__ ex, int64_t NE,
                                                   int64_t per, int64_t RB, int64_t NS,
                                                   float* __restrict__ c_sc,
                                                   int* __restrict__ c_id) {
  TOPK_LDS;
  item_topk<D, KP, false>(E, W, B, V, first, k, ex, NE, per, RB, NS, c_sc, c_id, l_sc, l_id, l_ex,
                          AllowArgs{});
}

template <int D, int KP>
__global__ __launch_bounds__(256) void k_item_topk_allowed(
    const float* __restrict__ E, const float* __restrict__ W, int64_t B, int64_t V, int64_t first,
    int k, const int64_t* __restrict__ ex, int64_t NE, int64_t per, int64_t RB, int64_t NS,
    float* __restrict__ c_sc, int* __restrict__ c_id, AllowArgs al) {
  TOPK_LDS;
  item_topk<D, KP, true>(E, W, B, V, first, k, ex, NE, per, RB, NS, c_sc, c_id, l_sc, l_id, l_ex,
                         al);
}

// The capped lists: one more LDS array (a 16-bit group per entry: 16 KB at
// KP = 64, where int32 would not fit beside D = 256's stream buffers) and one
// more workspace array (the entries' groups as int32, -1 for none).
template <int D, int KP, bool kAllow>
__global__ __launch_bounds__(256) void k_item_topk_grouped(
    const float* __restrict__ E, const float* __restrict__ W, int64_t B, int64_t V, int64_t first,
    int k, const int64_t* __restrict__ ex, int64_t NE, int64_t per, int64_t RB, int64_t NS,
    float* __restrict__ c_sc, int* __restrict__ c_id, int* __restrict__ c_g, AllowArgs al,
    GroupArgs gr) {
  TOPK_LDS;
  __shared__ unsigned short l_g[KP * kWaves * kTile];
  item_topk<D, KP, kAllow, true>(E, W, B, V, first, k, ex, NE, per, RB, NS, c_sc, c_id, l_sc, l_id,
                                 l_ex, al, c_g, l_g, gr);
}

// The lists under a prior: the LDS of the kernel without one, to the byte (the
// prior lives in registers), so the grouped d = 256, KP = 64 instantiation
// stands where k_item_topk_grouped's does.  Instantiated for <kAllow, kGroup> =
// (0, 0), (1, 0) and (1, 1): a cap without a filter runs (1, 1) with al.words
// null.
template <int D, int KP, bool kAllow, bool kGroup>
__global__ __launch_bounds__(256) void k_item_topk_prior(
    const float* __restrict__ E, const float* __restrict__ W, int64_t B, int64_t V, int64_t first,
    int k, const int64_t* __restrict__ ex, int64_t NE, int64_t per, int64_t RB, int64_t NS,
    float* __restrict__ c_sc, int* __restrict__ c_id, int* __restrict__ c_g, AllowArgs al,
    GroupArgs gr, PriorArgs pa) {
  TOPK_LDS;
  if constexpr (kGroup) {
    __shared__ unsigned short l_g[KP * kWaves * kTile];
    item_topk<D, KP, kAllow, true, true>(E, W, B, V, first, k, ex, NE, per, RB, NS, c_sc, c_id,
                                         l_sc, l_id, l_ex, al, c_g, l_g, gr, pa);
  } else {
    item_topk<D, KP, kAllow, false, true>(E, W, B, V, first, k, ex, NE, per, RB, NS, c_sc, c_id,
                                          l_sc, l_id, l_ex, al, nullptr, nullptr, gr, pa);
  }
}

// One wave per row: the row's S lists of k candidates (all ids distinct: the
// splits partition the items) merged into the k best in order.  Turn t takes
// the best candidate that the previous turn's pick beats, so nothing is
// marked; the reduction over lanes uses the full comparison, so the result
// does not depend on which lane held which candidate.  Empty slots and turns
// that find nothing give id -1, score -inf.
__global__ __launch_bounds__(256) void k_topk_rows(const float* __restrict__ c_sc,
                                                   const int* __restrict__ c_id, int64_t S,
                                                   int64_t B, int k, int64_t* __restrict__ ids,
                                                   float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t n = S * k;
  float ps = INFINITY, my_s = -INFINITY;
  int pid = -1, my_id = kNoItem;   // previous pick: beats every candidate at first
  for (int t = 0; t < k; ++t) {
    float bs = -INFINITY;
    int bid = kNoItem;
    if (pid != kNoItem) {
      for (int64_t c = lane; c < n; c += 64) {
        const int64_t sp = c / k, i = c - sp * k;
        const float s = c_sc[(sp * B + b) * k + i];
        const int id = c_id[(sp * B + b) * k + i];
        if (beats(ps, pid, s, id) && beats(s, id, bs, bid)) {
          bs = s;
          bid = id;
        }
      }
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) {
        const float os = __shfl_xor(bs, sh);
        const int oid = __shfl_xor(bid, sh);
        if (beats(os, oid, bs, bid)) {
          bs = os;
          bid = oid;
        }
      }
    }
    ps = bs;
    pid = bid;
    if (lane == t) {
      my_s = bs;
      my_id = bid;
    }
  }
  if (lane < k) {
    ids[b * k + lane] = my_id == kNoItem ? -1 : (int64_t)my_id;
    scores[b * k + lane] = my_s;
  }
}

// k_topk_rows under the cap: the walk over the row's S k candidates in order
// that takes a candidate unless m of its group were taken.  Still k turns: pick
// t's group sits on lane t, its count among the picks is a ballot, and when a
// pick fills its group the next turn's scan retires that group's remaining
// candidates in the row's own workspace slice (they become empty slots; a lane
// re-reads only what it wrote itself), so a full group never costs a turn.  At
// most one group fills per turn.  Group -1 is never counted.
__global__ __launch_bounds__(256) void k_topk_rows_grouped(float* __restrict__ c_sc,
                                                           int* __restrict__ c_id,
                                                           const int* __restrict__ c_g, int64_t S,
                                                           int64_t B, int k, int m,
                                                           int64_t* __restrict__ ids,
                                                           float* __restrict__ scores) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t n = S * k;
  float ps = INFINITY, my_s = -INFINITY;
  int pid = -1, my_id = kNoItem, my_g = -1;
  int full = -2;   // the group that the previous pick filled (-2: none)
  for (int t = 0; t < k; ++t) {
    float bs = -INFINITY;
    int bid = kNoItem, bg = -1;
    if (pid != kNoItem) {
      for (int64_t c = lane; c < n; c += 64) {
        const int64_t sp = c / k, i = c - sp * k, at = (sp * B + b) * k + i;
        const float s = c_sc[at];
        const int id = c_id[at];
        const int g = c_g[at];
        if (g == full) {
          c_sc[at] = -INFINITY;
          c_id[at] = kNoItem;
        } else if (beats(ps, pid, s, id) && beats(s, id, bs, bid)) {
          bs = s;
          bid = id;
          bg = g;
        }
      }
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) {
        const float os = __shfl_xor(bs, sh);
        const int oid = __shfl_xor(bid, sh);
        const int og = __shfl_xor(bg, sh);
        if (beats(os, oid, bs, bid)) {
          bs = os;
          bid = oid;
          bg = og;
        }
      }
    }
    ps = bs;
    pid = bid;
    const bool taken = bid != kNoItem && bg >= 0;
    const int same = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < t && my_g == bg));
    full = taken && same + 1 >= m ? bg : -2;
    if (lane == t) {
      my_s = bs;
      my_id = bid;
      my_g = taken ? bg : -1;
    }
  }
  if (lane < k) {
    ids[b * k + lane] = my_id == kNoItem ? -1 : (int64_t)my_id;
    scores[b * k + lane] = my_s;
  }
}

// ---- score matrix (full_sort_predict) and CE gradient of the logits -------------
// X[b][v], lane = item column v, rows b in registers, stored as 128-B row
// segments.  kProbs: stores P[b][v] = (exp(x - lse[b]) - [v + v_off ==
// target[b]]) * dloss / B instead (the logits' gradient, consumed by two
// library GEMMs: dseq = P W, ditems = P^T seq).  out has row stride ld.
template <int D, bool kProbs>
__global__ __launch_bounds__(256) void k_item_scores(const float* __restrict__ E,
                                                     const float* __restrict__ W, int64_t B,
                                                     int64_t V, int64_t per, int64_t RB, int64_t NS,
                                                     float* __restrict__ out, int64_t ld,
                                                     const float* __restrict__ lse,
                                                     const int64_t* __restrict__ tgt,
                                                     const float* __restrict__ dloss, float inv_n,
                                                     int64_t v_off) {
  constexpr int KH = D / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b0 = (pl.rb * kWaves + wave) * kTile;
  float ea[KH];
  ld_half<KH>(ea, E + min(b0 + j, B - 1) * D, h);
  float lr[kProbs ? 16 : 1];
  int64_t tr[kProbs ? 16 : 1];
  float g = 0.0f;
  if constexpr (kProbs) {
    g = dloss[0] * inv_n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = min(b0 + crow(r, h), B - 1);
      lr[r] = lse[row];
      tr[r] = tgt[row] - v_off;
    }
  }
  stream_tiles<D, false>(W, V, per, pl.split, nullptr, nullptr,
                         [&](int64_t t, const float* tile, const float*, const int64_t*) {
    const int64_t v = t * kTile + j;
    const f32x16 x = lds_dot<D, KH, false>(tile, j, h, ea);
    if (v < V) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = b0 + crow(r, h);
        float val = x[r];
        if constexpr (kProbs) val = (fexp(x[r] - lr[r]) - (v == tr[r] ? 1.0f : 0.0f)) * g;
        if (row < B) out[row * ld + v] = val;
      }
    }
  });
}

// ---- the f16 pipe: two-part split operands -------------------------------------
// The CE forward and the logits' gradient (the training step's two scoring
// kernels) run on v_mfma_f32_32x32x16_f16, 16x the fp32 MFMA rate, with
// fp32-level accuracy (the GEMMs' scheme, csrc/gemm_half.hip): each row x of
// seq and of the item table is scaled by an exact power of two and split,
//   x = 2^(e - kTS) (x0 + x1), x0 = f16(x 2^(kTS - e)), x1 = f16(x 2^(kTS - e) - x0),
// e the frexp exponent of max|x| (the row max lands in [2^13, 2^14)): 22
// significant bits.  A score is x0.y0 + x0.y1 + x1.y0 accumulated in fp32
// (each product exact; the dropped x1.y1 <= 2^-22 relative), un-scaled by
// v_ldexp (exact).  Image row = [x0 (D halfs) | x1 (D halfs)] = the fp32
// row's D*4 bytes, so the tile DMA and its swizzle are unchanged; the
// exponents are one int32 per row beside it.  Both kernels run the three
// products in the same order with the item parts first, so the forward's
// log-sum-exp and the gradient kernel see bit-identical logits.
// The rank / score kernels (evaluation) stay on the fp32 pipe: their target
// score replays the exact fma chain (k_target_dot).
constexpr int kTS = 14;

// one wave per row: max|x| over the row, then the two planes (4 values per
// lane and pass)
__global__ __launch_bounds__(256) void k_split_rows_h(const float* __restrict__ X, int64_t N, int D,
                                                      _Float16* __restrict__ img,
                                                      int* __restrict__ ex) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= N) return;
  const float4* x = reinterpret_cast<const float4*>(X + r * D);
  const int nq = D / 4;
  float m = 0.0f;
  for (int q = lane; q < nq; q += 64) {
    const float4 v = x[q];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  const int e = exp_of(m);
  _Float16* h0 = img + r * 2 * D;
  _Float16* h1 = h0 + D;
  for (int q = lane; q < nq; q += 64) {
    const float4 v = x[q];
    const float t[4] = {v.x, v.y, v.z, v.w};
    _Float16 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float sv = __builtin_amdgcn_ldexpf(t[i], kTS - e);   // exact (power of two)
      a[i] = (_Float16)sv;
      b[i] = (_Float16)(sv - (float)a[i]);
    }
    *reinterpret_cast<f16x4*>(h0 + 4 * q) = f16x4{a[0], a[1], a[2], a[3]};
    *reinterpret_cast<f16x4*>(h1 + 4 * q) = f16x4{b[0], b[1], b[2], b[3]};
  }
  if (lane == 0) ex[r] = e;
}

// The same split with the 32-row group maxima of x as a side output (the
// weight-gradient GEMM's operand scales: rb_group_absmax's values, bit for
// bit): 32 rows per workgroup, a wave's 8 rows loaded together (d <= 256:
// one float4 per lane and row), the group's max over the four waves in LDS.
__global__ __launch_bounds__(256) void k_split_rows_hg(const float* __restrict__ X, int64_t N,
                                                       int D, _Float16* __restrict__ img,
                                                       int* __restrict__ ex,
                                                       float* __restrict__ gmax) {
  __shared__ float sm[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 32 + w * 8;
  const int nq = D / 4;
  const float4* x = reinterpret_cast<const float4*>(X);
  float4 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    v[j] = (r0 + j < N && lane < nq) ? x[(r0 + j) * nq + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
  float wm = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float m = fmaxf(fmaxf(fabsf(v[j].x), fabsf(v[j].y)), fmaxf(fabsf(v[j].z), fabsf(v[j].w)));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    wm = fmaxf(wm, m);
    const int64_t r = r0 + j;
    if (r < N) {
      const int e = exp_of(m);
      if (lane < nq) {
        const float t[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        _Float16 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float sv = __builtin_amdgcn_ldexpf(t[i], kTS - e);
          a[i] = (_Float16)sv;
          b[i] = (_Float16)(sv - (float)a[i]);
        }
        _Float16* h0 = img + r * 2 * D;
        *reinterpret_cast<f16x4*>(h0 + 4 * lane) = f16x4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<f16x4*>(h0 + D + 4 * lane) = f16x4{b[0], b[1], b[2], b[3]};
      }
      if (lane == 0) ex[r] = e;
    }
  }
  if (lane == 0) sm[w] = wm;
  __syncthreads();
  if (threadIdx.x == 0) gmax[blockIdx.x] = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// this lane's register operand: row `row` of an image, k-blocks 16s + 8h ..
// 16s + 8h + 7 of both planes (the MFMA fragment of step s)
template <int D>
__device__ __forceinline__ void ld_frag_h(f16x8 (&p0)[D / 16], f16x8 (&p1)[D / 16],
                                          const _Float16* img, int64_t row, int h) {
  const _Float16* r = img + row * 2 * D + 8 * h;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    p0[s] = *reinterpret_cast<const f16x8*>(r + 16 * s);
    p1[s] = *reinterpret_cast<const f16x8*>(r + D + 16 * s);
  }
}

// X = items . seq over the full depth, item row j's fragments from the
// swizzled LDS image tile, the other operand's from registers (kTileIsA:
// the tile supplies A — rows of X are items — else B).  Per k16 step the
// three products item1.seq0, item0.seq1, item0.seq0, in that order in both
// orientations.  The tile reads run one step ahead of the MFMAs.
template <int D, bool kTileIsA>
__device__ __forceinline__ f32x16 lds_dot_h(const float* tile, int j, int h, const f16x8 (&r0)[D / 16],
                                            const f16x8 (&r1)[D / 16]) {
  constexpr int KS = D / 16;
  const float* row = tile + j * D;
  int sw = j % Stream<D>::NS;
  asm volatile("" : "+v"(sw));
  auto rd = [&](int slot) {
    return __builtin_bit_cast(f16x8, *reinterpret_cast<const float4*>(row + ((slot ^ sw) << 2)));
  };
  f16x8 w0[KS], w1[KS];
  w0[0] = rd(h);
  w1[0] = rd(D / 8 + h);
  f32x16 acc = {};
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s + 1 < KS) {
      w0[s + 1] = rd(2 * (s + 1) + h);
      w1[s + 1] = rd(D / 8 + 2 * (s + 1) + h);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (kTileIsA) {
      acc = mfma_h(w1[s], r0[s], acc);
      acc = mfma_h(w0[s], r1[s], acc);
      acc = mfma_h(w0[s], r0[s], acc);
    } else {
      // (the roles swapped: not mfma3_h's operand order)
      acc = mfma_h(r0[s], w1[s], acc);
      acc = mfma_h(r1[s], w0[s], acc);
      acc = mfma_h(r0[s], w0[s], acc);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  return acc;
}

// k_ce_fwd on the f16 pipe: the same tiles, partials and target capture;
// the item exponents of each tile ride along in LDS (rows crow(r, h): four
// 16-B reads)
template <int D>
__global__ __launch_bounds__(256) void k_ce_fwd_h(const _Float16* __restrict__ Ei,
                                                  const int* __restrict__ Ee,
                                                  const _Float16* __restrict__ Wi,
                                                  const int* __restrict__ We,
                                                  const int64_t* __restrict__ tgt, int64_t B,
                                                  int64_t V, int64_t per, int64_t RB, int64_t NS,
                                                  float* __restrict__ m_part,
                                                  float* __restrict__ s_part,
                                                  float* __restrict__ ts,
                                                  unsigned* __restrict__ ticket) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *ticket = 0u;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b = (pl.rb * kWaves + wave) * kTile + j;
  const int64_t bc = min(b, B - 1);
  f16x8 e0[D / 16], e1[D / 16];
  ld_frag_h<D>(e0, e1, Ei, bc, h);
  const int eb = Ee[bc] - 2 * kTS;
  const int64_t tb = tgt[bc];
  float m = -INFINITY, s = 0.0f, tsv = 0.0f;
  bool has_ts = false;
  stream_tiles<D, 2>(reinterpret_cast<const float*>(Wi), V, per, pl.split,
                     reinterpret_cast<const float*>(We), nullptr,
                     [&](int64_t t, const float* tile, const float* ebuf, const int64_t*) {
    const int64_t v0 = t * kTile;
    f32x16 x = lds_dot_h<D, true>(tile, j, h, e0, e1);
    const int4* ev = reinterpret_cast<const int4*>(ebuf);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int4 q = ev[2 * g + h];   // items 8g + 4h .. 8g + 4h + 3 = rows crow(4g .. 4g + 3, h)
      x[4 * g] = __builtin_amdgcn_ldexpf(x[4 * g], q.x + eb);
      x[4 * g + 1] = __builtin_amdgcn_ldexpf(x[4 * g + 1], q.y + eb);
      x[4 * g + 2] = __builtin_amdgcn_ldexpf(x[4 * g + 2], q.z + eb);
      x[4 * g + 3] = __builtin_amdgcn_ldexpf(x[4 * g + 3], q.w + eb);
    }
    const int hi = rel32(V, v0), tt = rel32(tb, v0);
    if (hi >= kTile) {
#pragma unroll
      for (int r = 0; r < 16; ++r) lse_push(m, s, x[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (crow(r, h) < hi) lse_push(m, s, x[r]);
    }
    if (tt >= 0 && tt < kTile) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (crow(r, h) == tt) {
          tsv = x[r];
          has_ts = true;
        }
    }
  });
  if (has_ts && b < B) ts[b] = tsv;
  lse_merge(m, s, __shfl_xor(m, 32), __shfl_xor(s, 32));
  if (h == 0 && b < B) {
    m_part[pl.split * B + b] = m;
    s_part[pl.split * B + b] = s;
  }
}

// k_item_scores<D, true> on the f16 pipe (the logits' gradient P): seq rows
// in registers (A), item tiles streamed (B) with their exponents.  TR: P^T
// [V, ld] instead (each lane's 16 rows as four 16-B pieces of its item's
// row) and every 32-item group's max |P| (atomicMax into gmax, zeroed by the
// caller): the operands of the input gradients as f16x3 GEMMs
// (scoring._bwd_slices).  MODE 0: P; 1: P^T + gmax; 2: both layouts (P into
// out2 [B, ld2]), gmax and every 32-row group's max |P| (bmax, atomicMax) —
// the operands of both input gradients as rb_gemm_tn_h products
// (scoring._bwd_f16).
// ROWS (rb_item_ce_probs_h_rows / _both_rows): a target of -1 is an ignored
// row; its lse is taken as +inf, so exp(x - lse) = 0 for its finite logits and
// its P entries are exactly 0 (nothing added to either group maximum).
template <int D, int MODE, bool ROWS = false>
__global__ __launch_bounds__(256) void k_ce_probs_h(const _Float16* __restrict__ Ei,
                                                    const int* __restrict__ Ee,
                                                    const _Float16* __restrict__ Wi,
                                                    const int* __restrict__ We, int64_t B,
                                                    int64_t V, int64_t per, int64_t RB, int64_t NS,
                                                    float* __restrict__ out, int64_t ld,
                                                    const float* __restrict__ lse,
                                                    const int64_t* __restrict__ tgt,
                                                    const float* __restrict__ dloss, float inv_n,
                                                    int64_t v_off, float* __restrict__ gmax,
                                                    float* __restrict__ out2, int64_t ld2,
                                                    float* __restrict__ bmax) {
  constexpr bool TR = MODE != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
  Place pl;
  if (!place(RB, NS, pl)) return;
  const int64_t b0 = (pl.rb * kWaves + wave) * kTile;
  f16x8 e0[D / 16], e1[D / 16];
  ld_frag_h<D>(e0, e1, Ei, min(b0 + j, B - 1), h);
  // per output row (registers r): lse, the target's column in this slice
  // (-1 outside it; V < 2^31) and the row's exponent — 48 registers, int32
  // where possible so two waves fit per SIMD
  float lr[16];
  int tr[16], er[16];
  const float g = dloss[0] * inv_n;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t row = min(b0 + crow(r, h), B - 1);
    const int64_t t = tgt[row];
    lr[r] = (ROWS && t == -1) ? INFINITY : lse[row];
    const int64_t tv = t - v_off;
    tr[r] = (tv >= 0 && tv < V) ? (int)tv : -1;
    er[r] = Ee[row] - 2 * kTS;
  }
  const bool full = b0 + kTile <= B;
  float mb = 0.0f;   // MODE 2: max |P| over the wave's rows and tiles
  stream_tiles<D, 2>(reinterpret_cast<const float*>(Wi), V, per, pl.split,
                     reinterpret_cast<const float*>(We), nullptr,
                     [&](int64_t t, const float* tile, const float* ebuf, const int64_t*) {
    const int v = (int)(t * kTile) + j;
    const f32x16 x = lds_dot_h<D, false>(tile, j, h, e0, e1);
    const int ev = reinterpret_cast<const int*>(ebuf)[j];
    if constexpr (!TR) {
      if (v < V) {
        float* o = out + (b0 + 4 * h) * ld + v;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = crow(r, 0);   // row - b0 - 4h
          const float xs = __builtin_amdgcn_ldexpf(x[r], ev + er[r]);
          const float val = (fexp(xs - lr[r]) - (v == tr[r] ? 1.0f : 0.0f)) * g;
          if (full || b0 + 4 * h + rr < B) o[rr * ld] = val;
        }
      }
    } else {
      float m = 0.0f;
      if (v < V) {
        float* o = out + (int64_t)v * ld + b0 + 4 * h;
#pragma unroll
        for (int q = 0; q < 4; ++q) {   // rows b0 + 8q + 4h + 0..3
          rb_f32x4 val4;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int r = 4 * q + u;
            const float xs = __builtin_amdgcn_ldexpf(x[r], ev + er[r]);
            const bool in = full || b0 + 8 * q + 4 * h + u < B;
            val4[u] = in ? (fexp(xs - lr[r]) - (v == tr[r] ? 1.0f : 0.0f)) * g : 0.0f;
            m = fmaxf(m, fabsf(val4[u]));
          }
          if (full) {
            *reinterpret_cast<rb_f32x4*>(o + 8 * q) = val4;
          } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (b0 + 8 * q + 4 * h + u < B) o[8 * q + u] = val4[u];
          }
          if constexpr (MODE == 2) {   // the same values row-major: out2[b][v]
            float* o2 = out2 + (b0 + 8 * q + 4 * h) * ld2 + v;
#pragma unroll
            for (int u = 0; u < 4; ++u)
              if (full || b0 + 8 * q + 4 * h + u < B) o2[u * ld2] = val4[u];
          }
        }
      }
      if constexpr (MODE == 2) mb = fmaxf(mb, m);
#pragma unroll
      for (int sh = 32; sh >= 1; sh >>= 1) m = fmaxf(m, __shfl_xor(m, sh));
      if (lane == 0)   // non-negative floats order as their bit patterns
        atomicMax(reinterpret_cast<int*>(gmax) + t, __float_as_int(m));
    }
  });
  if constexpr (MODE == 2) {
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) mb = fmaxf(mb, __shfl_xor(mb, sh));
    if (lane == 0 && b0 < B) atomicMax(reinterpret_cast<int*>(bmax) + b0 / kTile, __float_as_int(mb));
    // out2's padding columns [V, ld2) of the wave's rows: zeros (the first
    // item split's workgroups; no separate fill launch)
    if (pl.split == 0 && ld2 > V) {
      for (int r = 0; r < kTile && b0 + r < B; ++r)
        for (int64_t v = V + lane; v < ld2; v += 64) out2[(b0 + r) * ld2 + v] = 0.0f;
    }
  }
}

// ---- host side ---------------------------------------------------------------------
size_t al256(size_t x) { return (x + 255) & ~size_t(255); }

// the regions of a workspace, back to back from 256-B boundaries
struct WsCursor {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t r = off;
    off = al256(off + bytes);
    return r;
  }
};

struct Grid2 {
  int64_t blocks, splits, per;  // blocks over the fixed axis, splits of the streamed axis
  unsigned wgs() const { return (unsigned)(blocks * ((splits + 7) / 8 * 8)); }  // see place()
};

// fixed axis: n_fixed rows (kWaves*kTile per workgroup); streamed axis: n_stream tiles
Grid2 plan(int64_t n_fixed, int64_t n_stream_tiles) {
  const int64_t blocks = (n_fixed + kWaves * kTile - 1) / (kWaves * kTile);
  int64_t s = (kTargetWgs + blocks - 1) / blocks;
  s = std::max<int64_t>(1, std::min<int64_t>(s, n_stream_tiles));
  const int64_t per = (n_stream_tiles + s - 1) / s;
  return {blocks, (n_stream_tiles + per - 1) / per, per};
}

int64_t ntiles(int64_t n) { return (n + kTile - 1) / kTile; }

struct CeWs {
  size_t ts, m, s, rows, ticket, de, dw, total;
};

CeWs ce_layout(int64_t B, int64_t V, int64_t D) {
  const Grid2 f = plan(B, ntiles(V)), w = plan(V, ntiles(B));
  CeWs o{};
  WsCursor c;
  o.ts = c.take(B * 4);
  o.m = c.take(f.splits * B * 4);
  o.s = c.take(f.splits * B * 4);
  o.rows = c.take(B * 4);
  o.ticket = c.take(4);
  o.de = c.take(f.splits * B * D * 4);
  o.dw = c.take(w.splits * V * D * 4);
  o.total = c.off;
  return o;
}

struct RankWs {
  size_t ts, gt, eq, total;
};

RankWs rank_layout(int64_t B, int64_t V) {
  const Grid2 f = plan(B, ntiles(V));
  RankWs o{};
  WsCursor c;
  o.ts = c.take(B * 4);
  o.gt = c.take(f.splits * B * 4);
  o.eq = c.take(f.splits * B * 4);
  o.total = c.off;
  return o;
}

struct TopkWs {
  size_t sc, id, g, total;
};

// grouped: the third array (each entry's group) of rb_item_topk_grouped
TopkWs topk_layout(int64_t B, int64_t V, int64_t k, bool grouped = false) {
  const Grid2 f = plan(B, ntiles(V));
  TopkWs o{};
  WsCursor c;
  o.sc = c.take(f.splits * B * k * 4);
  o.id = c.take(f.splits * B * k * 4);
  if (grouped) o.g = c.take(f.splits * B * k * 4);
  o.total = c.off;
  return o;
}

// f(std::integral_constant<int, D>{}) for the kernels' feature depths; any
// other d is an error
template <class F>
int for_item_dim(int64_t D, F&& f) {
  if (dispatch_int<16, 32, 64, 128, 256>((int)D, f)) return 0;
  return fail("item scores: d must be 16, 32, 64, 128 or 256");
}

// The one launch of k_ce_probs_h.  The kernel's first output is P^T whenever it
// writes one (MODE 1, 2), with P second in MODE 2; MODE 0 writes P alone.
template <int D, int MODE, bool ROWS>
void probs_h_launch(const void* Ei, const int* Ee, const void* Wi, const int* We, int64_t B,
                    int64_t V, const Grid2& g, const CeProbsOut& o, const float* lse,
                    const int64_t* tgt, const float* dloss, float inv_n, int64_t v_off,
                    hipStream_t st) {
  constexpr bool TR = MODE != 0, BOTH = MODE == 2;
  hipLaunchKernelGGL((k_ce_probs_h<D, MODE, ROWS>), dim3(g.wgs()), dim3(256), 0, st,
                     (const _Float16*)Ei, Ee, (const _Float16*)Wi, We, B, V, g.per, g.blocks,
                     g.splits, TR ? o.pt : o.p, TR ? o.ldt : o.ld, lse, tgt, dloss, inv_n, v_off,
                     TR ? o.item_max : nullptr, BOTH ? o.p : nullptr, BOTH ? o.ld : (int64_t)0,
                     BOTH ? o.row_max : nullptr);
}

// mode: 0 P, 1 P^T, 2 both (launch_item_ce_probs_h rejects rows with mode 1)
template <int D, class... Args>
void probs_h_t(int mode, bool rows, Args... a) {
  if (rows && mode == 2) probs_h_launch<D, 2, true>(a...);
  else if (rows) probs_h_launch<D, 0, true>(a...);
  else if (mode == 2) probs_h_launch<D, 2, false>(a...);
  else if (mode == 1) probs_h_launch<D, 1, false>(a...);
  else probs_h_launch<D, 0, false>(a...);
}

// The forward's two passes over one workspace: `partials` (k_ce_fwd or
// k_ce_fwd_h, by d) leaves each item split's running max and sum, and
// k_ce_rows<ROWS> folds them into lse and the loss.
template <bool ROWS, class Partials>
int ce_fwd_passes(const char* fn, const int64_t* tgt, int64_t B, int64_t V, int64_t D, float* lse,
                  float* loss, void* ws, int64_t ws_bytes, float inv_n, int accumulate,
                  hipStream_t st, Partials partials) {
  const CeWs L = ce_layout(B, V, D);
  if (ws_bytes < (int64_t)L.total) return fail((std::string(fn) + ": workspace too small").c_str());
  char* w = static_cast<char*>(ws);
  float* ts = reinterpret_cast<float*>(w + L.ts);
  float* m = reinterpret_cast<float*>(w + L.m);
  float* s = reinterpret_cast<float*>(w + L.s);
  float* rows = reinterpret_cast<float*>(w + L.rows);
  unsigned* ticket = reinterpret_cast<unsigned*>(w + L.ticket);
  const Grid2 g = plan(B, ntiles(V));
  if (int rc = partials(g, m, s, ts, ticket)) return rc;
  hipLaunchKernelGGL(k_ce_rows<ROWS>, dim3((unsigned)((B + 63) / 64)), dim3(256), 0, st, m, s,
                     g.splits, ts, tgt, B, V, lse, rows, ticket, loss, inv_n, accumulate);
  return launch_status(fn);
}

void sum_parts(const float* parts, int64_t P, int64_t n, float* out, hipStream_t st) {
  const int64_t threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_sum_parts, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, parts,
                     P, n, out);
}

}  // namespace

int64_t item_ce_workspace_bytes(int64_t B, int64_t V, int64_t D) {
  return (int64_t)ce_layout(B, V, D).total;
}

int64_t item_rank_workspace_bytes(int64_t B, int64_t V) {
  return (int64_t)rank_layout(B, V).total;
}

int launch_item_ce_fwd(const float* E, const float* W, const int64_t* tgt, int64_t B, int64_t V,
                       int64_t D, float* lse, float* loss, void* ws, int64_t ws_bytes,
                       hipStream_t st) {
  return ce_fwd_passes<false>(
      "rb_item_ce_fwd", tgt, B, V, D, lse, loss, ws, ws_bytes, 0.0f, 0, st,
      [&](const Grid2& g, float* m, float* s, float* ts, unsigned* ticket) {
        return for_item_dim(D, [&](auto dc) {
          hipLaunchKernelGGL(k_ce_fwd<dc>, dim3(g.wgs()), dim3(256), 0, st, E, W, tgt, B, V, g.per,
                             g.blocks, g.splits, m, s, ts, ticket);
        });
      });
}

int launch_item_ce_bwd(const float* E, const float* W, const int64_t* tgt, const float* lse,
                       const float* dloss, int64_t B, int64_t V, int64_t D, float* dE, float* dW,
                       void* ws, int64_t ws_bytes, hipStream_t st) {
  const CeWs L = ce_layout(B, V, D);
  if (ws_bytes < (int64_t)L.total) return fail("rb_item_ce_bwd: workspace too small");
  char* w = static_cast<char*>(ws);
  const float inv_n = 1.0f / (float)B;
  if (dE) {
    float* part = reinterpret_cast<float*>(w + L.de);
    const Grid2 g = plan(B, ntiles(V));
    if (int rc = for_item_dim(D, [&](auto dc) {
          hipLaunchKernelGGL(k_ce_bwd_seq<dc>, dim3(g.wgs()), dim3(256), 0, st, E, W, lse, tgt,
                             dloss, inv_n, B, V, g.per, g.blocks, g.splits, part);
        }))
      return rc;
    sum_parts(part, g.splits, B * D, dE, st);
  }
  if (dW) {
    float* part = reinterpret_cast<float*>(w + L.dw);
    const Grid2 g = plan(V, ntiles(B));
    if (int rc = for_item_dim(D, [&](auto dc) {
          hipLaunchKernelGGL(k_ce_bwd_item<dc>, dim3(g.wgs()), dim3(256), 0, st, E, W, lse, tgt,
                             dloss, inv_n, B, V, g.per, g.blocks, g.splits, part);
        }))
      return rc;
    sum_parts(part, g.splits, V * D, dW, st);
  }
  return launch_status("rb_item_ce_bwd");
}

// rb_item_rank, _allowed and _prior (fn names the caller for the messages; al,
// pa: null where the option is off): one workspace, one plan; a prior, with a
// filter or not, has kernels of its own
int launch_item_rank(const char* fn, const float* E, const float* W, const int64_t* tgt,
                     int64_t B, int64_t V, int64_t D, int64_t first, int64_t* n_gt,
                     int64_t* n_eq, void* ws, int64_t ws_bytes, const AllowArgs* al,
                     const PriorArgs* pa, hipStream_t st) {
  const RankWs L = rank_layout(B, V);
  if (ws_bytes < (int64_t)L.total) return fail((std::string(fn) + ": workspace too small").c_str());
  char* w = static_cast<char*>(ws);
  float* ts = reinterpret_cast<float*>(w + L.ts);
  int* gt = reinterpret_cast<int*>(w + L.gt);
  int* eq = reinterpret_cast<int*>(w + L.eq);
  const Grid2 g = plan(B, ntiles(V));
  const dim3 rows((unsigned)((B + 255) / 256));
  if (int rc = for_item_dim(D, [&](auto dc) {
        if (pa) {
          const AllowArgs a = al ? *al : AllowArgs{};
          hipLaunchKernelGGL(k_target_dot_prior<dc>, rows, dim3(256), 0, st, E, W, tgt, B, V, ts,
                             a, *pa);
          const auto kernel = al ? k_item_rank_prior<dc, true> : k_item_rank_prior<dc, false>;
          hipLaunchKernelGGL(kernel, dim3(g.wgs()), dim3(256), 0, st, E, W, ts, tgt, B, V, first,
                             g.per, g.blocks, g.splits, gt, eq, a, *pa);
        } else if (al) {
          hipLaunchKernelGGL(k_target_dot_allowed<dc>, rows, dim3(256), 0, st, E, W, tgt, B, V, ts,
                             *al);
          hipLaunchKernelGGL(k_item_rank_allowed<dc>, dim3(g.wgs()), dim3(256), 0, st, E, W, ts,
                             tgt, B, V, first, g.per, g.blocks, g.splits, gt, eq, *al);
        } else {
          hipLaunchKernelGGL(k_target_dot<dc>, rows, dim3(256), 0, st, E, W, tgt, B, V, ts);
          hipLaunchKernelGGL(k_item_rank<dc>, dim3(g.wgs()), dim3(256), 0, st, E, W, ts, tgt, B, V,
                             first, g.per, g.blocks, g.splits, gt, eq);
        }
      }))
    return rc;
  hipLaunchKernelGGL(k_rank_rows, rows, dim3(256), 0, st, gt, eq, g.splits, ts, B, n_gt, n_eq);
  return launch_status(fn);
}

int64_t item_topk_workspace_bytes(int64_t B, int64_t V, int64_t k) {
  return (int64_t)topk_layout(B, V, k).total;
}

int64_t item_topk_grouped_workspace_bytes(int64_t B, int64_t V, int64_t k) {
  return (int64_t)topk_layout(B, V, k, true).total;
}

// rb_item_topk, _allowed, _grouped and _prior (fn names the caller for the
// messages; al, gr, pa: null where the option is off): one plan, one workspace
// but for the cap's third array, one selection launch and one merge launch
int launch_item_topk(const char* fn, const float* E, const float* W, int64_t B, int64_t V,
                     int64_t D, int64_t k, int64_t first, const int64_t* ex, int64_t NE,
                     int64_t* ids, float* scores, void* ws, int64_t ws_bytes,
                     const AllowArgs* al, const GroupArgs* gr, const PriorArgs* pa,
                     hipStream_t st) {
  const TopkWs L = topk_layout(B, V, k, gr != nullptr);
  if (ws_bytes < (int64_t)L.total) return fail((std::string(fn) + ": workspace too small").c_str());
  char* w = static_cast<char*>(ws);
  float* sc = reinterpret_cast<float*>(w + L.sc);
  int* id = reinterpret_cast<int*>(w + L.id);
  int* cg = gr ? reinterpret_cast<int*>(w + L.g) : nullptr;
  const Grid2 g = plan(B, ntiles(V));
  const AllowArgs a = al ? *al : AllowArgs{};
  if (int rc = for_item_dim(D, [&](auto dc) {
        // the kernel of the option set, at the candidate list's LDS capacity per
        // (row, split): 32 or 64
        const dim3 grid(g.wgs()), block(256);
        if (pa) {
          const auto kernel =
              gr ? (k <= 32 ? k_item_topk_prior<dc, 32, true, true>
                            : k_item_topk_prior<dc, 64, true, true>)
              : al ? (k <= 32 ? k_item_topk_prior<dc, 32, true, false>
                              : k_item_topk_prior<dc, 64, true, false>)
                   : (k <= 32 ? k_item_topk_prior<dc, 32, false, false>
                              : k_item_topk_prior<dc, 64, false, false>);
          hipLaunchKernelGGL(kernel, grid, block, 0, st, E, W, B, V, first, (int)k, ex, NE, g.per,
                             g.blocks, g.splits, sc, id, cg, a, gr ? *gr : GroupArgs{}, *pa);
        } else if (gr) {
          const auto kernel =
              al ? (k <= 32 ? k_item_topk_grouped<dc, 32, true> : k_item_topk_grouped<dc, 64, true>)
                 : (k <= 32 ? k_item_topk_grouped<dc, 32, false>
                            : k_item_topk_grouped<dc, 64, false>);
          hipLaunchKernelGGL(kernel, grid, block, 0, st, E, W, B, V, first, (int)k, ex, NE, g.per,
                             g.blocks, g.splits, sc, id, cg, a, *gr);
        } else if (al) {
          const auto kernel = k <= 32 ? k_item_topk_allowed<dc, 32> : k_item_topk_allowed<dc, 64>;
          hipLaunchKernelGGL(kernel, grid, block, 0, st, E, W, B, V, first, (int)k, ex, NE, g.per,
                             g.blocks, g.splits, sc, id, a);
        } else {
          const auto kernel = k <= 32 ? k_item_topk<dc, 32> : k_item_topk<dc, 64>;
          hipLaunchKernelGGL(kernel, grid, block, 0, st, E, W, B, V, first, (int)k, ex, NE, g.per,
                             g.blocks, g.splits, sc, id);
        }
      }))
    return rc;
  const dim3 rows((unsigned)((B + 3) / 4));
  if (gr)
    hipLaunchKernelGGL(k_topk_rows_grouped, rows, dim3(256), 0, st, sc, id, cg, g.splits, B,
                       (int)k, gr->m, ids, scores);
  else
    hipLaunchKernelGGL(k_topk_rows, rows, dim3(256), 0, st, sc, id, g.splits, B, (int)k, ids,
                       scores);
  return launch_status(fn);
}

int launch_item_ce_probs(const float* E, const float* W, const int64_t* tgt, const float* lse,
                         const float* dloss, int64_t B, int64_t V, int64_t D, int64_t v_off,
                         float* out, int64_t ld, hipStream_t st) {
  const Grid2 g = plan(B, ntiles(V));
  const float inv_n = 1.0f / (float)B;
  if (int rc = for_item_dim(D, [&](auto dc) {
        hipLaunchKernelGGL((k_item_scores<dc, true>), dim3(g.wgs()), dim3(256), 0, st, E, W, B, V,
                           g.per, g.blocks, g.splits, out, ld, lse, tgt, dloss, inv_n, v_off);
      }))
    return rc;
  return launch_status("rb_item_ce_probs");
}

int launch_item_split_h(const float* X, int64_t N, int64_t D, void* img, int* ex, float* gmax,
                        hipStream_t st) {
  if (gmax != nullptr) {
    hipLaunchKernelGGL(k_split_rows_hg, dim3((unsigned)((N + 31) / 32)), dim3(256), 0, st, X, N,
                       (int)D, (_Float16*)img, ex, gmax);
    return launch_status("rb_item_split_h");
  }
  hipLaunchKernelGGL(k_split_rows_h, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, X, N, (int)D,
                     (_Float16*)img, ex);
  return launch_status("rb_item_split_h");
}

// rows: rb_item_ce_fwd_h_rows (target -1 = ignored row, loss = sum * inv_n,
// added to loss[0] when accumulate); else rb_item_ce_fwd_h (inv_n unused)
int launch_item_ce_fwd_h(const void* Ei, const int* Ee, const void* Wi, const int* We,
                         const int64_t* tgt, int64_t B, int64_t V, int64_t D, float* lse,
                         float* loss, void* ws, int64_t ws_bytes, bool rows_mode, float inv_n,
                         int accumulate, hipStream_t st) {
  const auto partials = [&](const Grid2& g, float* m, float* s, float* ts, unsigned* ticket) {
    return for_item_dim(D, [&](auto dc) {
      hipLaunchKernelGGL(k_ce_fwd_h<dc>, dim3(g.wgs()), dim3(256), 0, st, (const _Float16*)Ei, Ee,
                         (const _Float16*)Wi, We, tgt, B, V, g.per, g.blocks, g.splits, m, s, ts,
                         ticket);
    });
  };
  if (rows_mode)
    return ce_fwd_passes<true>("rb_item_ce_fwd_h_rows", tgt, B, V, D, lse, loss, ws, ws_bytes,
                               inv_n, accumulate, st, partials);
  return ce_fwd_passes<false>("rb_item_ce_fwd_h", tgt, B, V, D, lse, loss, ws, ws_bytes, 0.0f, 0,
                              st, partials);
}

int launch_item_ce_probs_h(const void* Ei, const int* Ee, const void* Wi, const int* We,
                           const int64_t* tgt, const float* lse, const float* dloss, int64_t B,
                           int64_t V, int64_t D, int64_t v_off, const CeProbsOut& o,
                           hipStream_t st) {
  const int mode = o.pt ? (o.p ? 2 : 1) : 0;
  if (o.rows && mode == 1) return fail("rb_item_ce_probs_h_rows: no transposed-only form");
  static const char* const kNames[2][3] = {
      {"rb_item_ce_probs_h", "rb_item_ce_probs_h_t", "rb_item_ce_probs_h_both"},
      {"rb_item_ce_probs_h_rows", nullptr, "rb_item_ce_probs_h_both_rows"}};
  const Grid2 g = plan(B, ntiles(V));
  // the rows forms take the caller's normaliser, the others the batch mean
  const float inv_n = o.rows ? o.inv_n : 1.0f / (float)B;
  if (int rc = for_item_dim(D, [&](auto dc) {
        probs_h_t<dc>(mode, o.rows, Ei, Ee, Wi, We, B, V, g, o, lse, tgt, dloss, inv_n, v_off, st);
      }))
    return rc;
  return launch_status(kNames[o.rows][mode]);
}

int launch_item_scores(const float* E, const float* W, int64_t B, int64_t V, int64_t D,
                       float* out, hipStream_t st) {
  const Grid2 g = plan(B, ntiles(V));
  if (int rc = for_item_dim(D, [&](auto dc) {
        hipLaunchKernelGGL((k_item_scores<dc, false>), dim3(g.wgs()), dim3(256), 0, st, E, W, B, V,
                           g.per, g.blocks, g.splits, out, V, nullptr, nullptr, nullptr, 0.0f,
                           (int64_t)0);
      }))
    return rc;
  return launch_status("rb_item_scores");
}

}  // namespace rb

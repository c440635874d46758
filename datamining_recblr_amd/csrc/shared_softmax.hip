// shared_softmax.hip — sampled softmax at every packed row, the negatives
// shared by the rows of a sequence (include/recblr_pairs.h):
//
//   z0 = h_r . E[target_r],  z_j = h_r . E[neg[b, j]] + shift,
//   loss_r = logsumexp(z0, z_j ...) - z0,  mean over the live rows.
//
// The scores of a sequence are one small dense product H_s [len, d] .
// E_neg [n, d]^T on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).  Both
// operands are streamed as 16-B row fragments straight from global memory
// (the n table rows of a sequence stay in L1 / L2 for its row tiles), as the
// session kernels' gemm16 streams its weights.
//
//   rb_shared_softmax_fwd   a workgroup takes 64-row blocks of one sequence,
//                           a wave one 16-row tile of it: per 16-column tile
//                           the scores come out transposed (lane = row, the
//                           four registers = columns 4g + q), the log-sum-exp
//                           runs online in registers, and the mean over the
//                           live rows is loss_tail.h's;
//   rb_shared_softmax_bwd   two kernels.  k_ss_dh recomputes the same score
//                           tiles, forms p_j = exp(z_j - lse) in the MFMA's A
//                           layout and accumulates dh = P E_neg on the MFMA,
//                           then subtracts the target's row; k_ss_dneg (one
//                           workgroup per sequence and 16-column tile) stages
//                           64 rows of H in LDS, recomputes its [64, 16]
//                           scores and accumulates dneg = P^T H over the
//                           sequence's row blocks in order.
// No float atomics; every sum has a fixed order that depends on the row's
// sequence and its position in it only.
//
//   rb_shared_softmax_fwd_items / _bwd_items   the same three kernel bodies
//                           (kItems) with a per-item correction of the
//                           proposal: a live column of id j scores z_j = (h_r .
//                           E[j] + shift) + item_shift[j], one 4-byte gather
//                           per column and 16-row tile; a dead or out-of-range
//                           column reads nothing.
#include "common.h"
#include "loss_tail.h"

namespace rb {
namespace {

constexpr int kSsRows = 64;        // rows of a sequence per workgroup pass (4 waves x 16)
constexpr int kSsMaxBlocks = 64;   // row blocks a sequence is spread over at most
constexpr int kSsMaxDt = 14;       // d <= 224: 16-column tiles of a dh row
constexpr int kPtLd = 17;

struct SsSeq {
  int64_t beg, end, b;
  bool ok;
};

// sequence s of the plan; a malformed entry (rows outside [0, M), an empty
// range, a batch row outside [0, B)) is skipped: nothing of it is read
__device__ __forceinline__ SsSeq ss_seq(const int64_t* __restrict__ offsets,
                                        const int64_t* __restrict__ order, int64_t s, int64_t M,
                                        int64_t B) {
  SsSeq q;
  q.beg = offsets[s];
  q.end = offsets[s + 1];
  q.b = order[s];
  q.ok = q.beg >= 0 && q.end <= M && q.beg < q.end && q.b >= 0 && q.b < B;
  return q;
}

// D[i][j] = sum_k A[i][k] B[j][k] of two 16-row fragments (a, b: the lane's
// row (lane & 15) + 4 (lane >> 4) floats); D[i][j] sits in lane j + 16 g,
// register q with i = 4 g + q.  MFMA jj of a 16-wide k block sums k = kb + 4
// g + jj: a permuted but fixed order, the same whichever operand is A.
__device__ __forceinline__ rb_f32x4 ss_scores(const float* a, const float* b, int d) {
  rb_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int kb = 0; kb < d; kb += 16) {
    const rb_f32x4 x = *reinterpret_cast<const rb_f32x4*>(a + kb);
    const rb_f32x4 y = *reinterpret_cast<const rb_f32x4*>(b + kb);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x[j], y[j], acc, 0, 0, 0);
  }
  return acc;
}

// (m, s) <- the log-sum-exp state of both
__device__ __forceinline__ void ss_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;   // both empty
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

// the ids of columns nt * 16 + 4 g + q of batch row b's list (-1 past n)
__device__ __forceinline__ void ss_col_ids(const int64_t* __restrict__ neg, int64_t b, int n,
                                           int nt, int g, int64_t (&id)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int col = nt * 16 + 4 * g + q;
    id[q] = col < n ? neg[b * n + col] : -1;
  }
}

template <bool kItems>
__global__ void __launch_bounds__(256)
k_ss_fwd(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
         const int64_t* __restrict__ target, const int64_t* __restrict__ neg,
         const int64_t* __restrict__ offsets, const int64_t* __restrict__ order, int64_t M,
         int64_t B, int d, int64_t V, int n, int RB, float shift,
         const float* __restrict__ item_shift, float* __restrict__ lse,
         float* __restrict__ z0o, float* psum, int* pcnt, unsigned* ticket,
         float* __restrict__ loss, int64_t* __restrict__ n_live) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t s = blockIdx.x / RB;
  const int rb0 = blockIdx.x % RB;
  const int NT = (n + 15) >> 4;
  const SsSeq q = ss_seq(offsets, order, s, M, B);
  float wsum = 0.0f;
  int wcnt = 0;
  if (q.ok) {
    for (int64_t r0 = q.beg + (int64_t)rb0 * kSsRows + wave * 16; r0 < q.end;
         r0 += (int64_t)RB * kSsRows) {
      const int64_t row = r0 + c;
      const bool in = row < q.end;
      const int64_t rc = in ? row : q.end - 1;
      const int64_t t = target[rc];
      const bool live = in && t >= 0 && t < V;
      bool bad = in && (t < -1 || t >= V);
      const float* hb = h + rc * ldh + 4 * g;
      const float* tp = tab + (live ? t : 0) * d + 4 * g;
      float z0 = 0.0f;
      for (int kb = 0; kb < d; kb += 16) {
        const rb_f32x4 x = *reinterpret_cast<const rb_f32x4*>(hb + kb);
        const rb_f32x4 y = *reinterpret_cast<const rb_f32x4*>(tp + kb);
        z0 += (x[0] * y[0] + x[1] * y[1]) + (x[2] * y[2] + x[3] * y[3]);
      }
      z0 += __shfl_xor(z0, 16);
      z0 += __shfl_xor(z0, 32);
      float m = -INFINITY, sum = 0.0f;
      for (int nt = 0; nt < NT; ++nt) {
        const int ca = nt * 16 + c;
        const int64_t ida = ca < n ? neg[q.b * n + ca] : -1;
        const float* ap = tab + (ida >= 0 && ida < V ? ida : 0) * d + 4 * g;
        const rb_f32x4 acc = ss_scores(ap, hb, d);   // [column][row]: lane = row c
        int64_t id[4];
        ss_col_ids(neg, q.b, n, nt, g, id);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bad |= in && (id[k] < -1 || id[k] >= V);
          if (id[k] >= 0 && id[k] < V) {
            float z = acc[k] + shift;
            if constexpr (kItems) z += item_shift[id[k]];
            if (z > m) {
              sum = sum * expf(m - z) + 1.0f;
              m = z;
            } else {
              sum += expf(z - m);
            }
          }
        }
      }
      ss_merge(m, sum, __shfl_xor(m, 16), __shfl_xor(sum, 16));
      ss_merge(m, sum, __shfl_xor(m, 32), __shfl_xor(sum, 32));
      float l = z0;   // no live column: loss 0
      if (m != -INFINITY) {
        const float mn = fmaxf(m, z0);
        l = mn + logf(sum * expf(m - mn) + expf(z0 - mn));
      }
      if (in && g == 0) {
        lse[row] = l;
        z0o[row] = z0;
      }
      int bad_any = bad ? 1 : 0;   // a bad id in any of the row's four column groups
      bad_any |= __shfl_xor(bad_any, 16);
      bad_any |= __shfl_xor(bad_any, 32);
      float v = g == 0 ? (bad_any ? NAN : live ? l - z0 : 0.0f) : 0.0f;
      int cnt = g == 0 && live ? 1 : 0;
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) {
        v += __shfl_xor(v, o, 16);
        cnt += __shfl_xor(cnt, o, 16);
      }
      wsum += v;   // lane 0's is the tile's
      wcnt += cnt;
    }
  }
  mean_loss_tail<4>(wsum, wcnt, psum, pcnt, ticket, loss, n_live);   // a slot per wave
}

// dh_r = scale (sum_j p_rj E[neg_j] - (sum_j p_rj) E[target_r]), coef_r = -scale
// sum_j p_rj (sum_j p_j = 1 - p_0 without the cancellation)
template <bool kItems>
__global__ void __launch_bounds__(256)
k_ss_dh(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
        const int64_t* __restrict__ target, const int64_t* __restrict__ neg,
        const int64_t* __restrict__ offsets, const int64_t* __restrict__ order,
        const float* __restrict__ lse, const float* __restrict__ dloss,
        const int64_t* __restrict__ n_live, int64_t M, int64_t B, int d, int64_t V, int n, int RB,
        float shift, const float* __restrict__ item_shift, float* __restrict__ dh,
        float* __restrict__ coef) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int64_t s = blockIdx.x / RB;
  const int rb0 = blockIdx.x % RB;
  const int NT = (n + 15) >> 4, DT = d >> 4;
  const SsSeq q = ss_seq(offsets, order, s, M, B);
  if (!q.ok) return;
  const int64_t nl = n_live[0];
  const float scale = dloss[0] / (float)(nl > 0 ? nl : 1);
  for (int64_t r0 = q.beg + (int64_t)rb0 * kSsRows + wave * 16; r0 < q.end;
       r0 += (int64_t)RB * kSsRows) {
    const int64_t row = r0 + c;
    const bool in = row < q.end;
    const int64_t rc = in ? row : q.end - 1;
    const int64_t t = target[rc];
    const bool live = in && t >= 0 && t < V;
    const float* hb = h + rc * ldh + 4 * g;
    const float l = lse[rc];
    rb_f32x4 acc[kSsMaxDt];
#pragma unroll
    for (int dt = 0; dt < kSsMaxDt; ++dt) acc[dt] = rb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float psum = 0.0f;
    for (int nt = 0; nt < NT; ++nt) {
      const int ca = nt * 16 + c;
      const int64_t ida = ca < n ? neg[q.b * n + ca] : -1;
      const float* ap = tab + (ida >= 0 && ida < V ? ida : 0) * d + 4 * g;
      const rb_f32x4 z = ss_scores(ap, hb, d);   // [column][row]: lane = row c
      int64_t id[4];
      ss_col_ids(neg, q.b, n, nt, g, id);
      float p[4];
      const float* ep[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const bool ok = id[k] >= 0 && id[k] < V;
        float zk = z[k] + shift;
        if constexpr (kItems) {
          if (ok) zk += item_shift[id[k]];
        }
        p[k] = live && ok ? expf(zk - l) : 0.0f;
        psum += p[k];
        p[k] *= scale;
        ep[k] = tab + (ok ? id[k] : 0) * d + c;
      }
      // A = P [row][column 4 g + k], B = E [column 4 g + k][16 dt + c]
#pragma unroll
      for (int dt = 0; dt < kSsMaxDt; ++dt) {
        if (dt < DT) {
#pragma unroll
          for (int k = 0; k < 4; ++k)
            acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(p[k], ep[k][dt * 16], acc[dt], 0, 0, 0);
        }
      }
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    const float rcoef = live ? scale * psum : 0.0f;
    if (in && g == 0) coef[row] = -rcoef;
    const int tc = live ? (int)t : 0;
    // acc[dt][k]: row 4 g + k, column 16 dt + c
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float rk = __shfl(rcoef, 4 * g + k);
      const int tk = __shfl(tc, 4 * g + k);
      const int lk = __shfl((int)live, 4 * g + k);
      const int64_t rw = r0 + 4 * g + k;
      if (rw >= q.end) continue;
      const float* er = tab + (int64_t)tk * d + c;
#pragma unroll
      for (int dt = 0; dt < kSsMaxDt; ++dt) {
        if (dt < DT) dh[rw * d + dt * 16 + c] = lk ? acc[dt][k] - rk * er[dt * 16] : 0.0f;
      }
    }
  }
}

// dneg[b, j, :] = scale sum_{r in s} p_rj h_r for the 16 columns of tile nt:
// the sequence's rows in blocks of 64 (Hs), wave w scores tile w of the block
// ([row][column]: lane = column c) and leaves P in Pt; then wave w owns the
// 16-column tiles dt = w, w + 4 ... of dneg's d and adds the block's four row
// tiles in order.
template <bool kItems>
__global__ void __launch_bounds__(256)
k_ss_dneg(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
          const int64_t* __restrict__ target, const int64_t* __restrict__ neg,
          const int64_t* __restrict__ offsets, const int64_t* __restrict__ order,
          const float* __restrict__ lse, const float* __restrict__ dloss,
          const int64_t* __restrict__ n_live, int64_t M, int64_t B, int d, int64_t V, int n,
          float shift, const float* __restrict__ item_shift, float* __restrict__ dneg) {
  extern __shared__ float ss_smem[];
  const int ldH = d + 4;
  float* Hs = ss_smem;                  // [64][ldH]
  float* Pt = Hs + kSsRows * ldH;       // [64][kPtLd]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int NT = (n + 15) >> 4, DT = d >> 4, dv = d >> 2;
  const int64_t s = blockIdx.x / NT;
  const int nt = blockIdx.x % NT;
  const SsSeq q = ss_seq(offsets, order, s, M, B);
  if (!q.ok) return;
  const int64_t nl = n_live[0];
  const float scale = dloss[0] / (float)(nl > 0 ? nl : 1);
  const int ca = nt * 16 + c;
  const int64_t ida = ca < n ? neg[q.b * n + ca] : -1;
  const bool oka = ida >= 0 && ida < V;
  const float* ap = tab + (oka ? ida : 0) * d + 4 * g;
  float isa = 0.0f;   // the lane's column's item_shift
  if constexpr (kItems) {
    if (oka) isa = item_shift[ida];
  }
  rb_f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = rb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int64_t blk = q.beg; blk < q.end; blk += kSsRows) {
    for (int e = threadIdx.x; e < kSsRows * dv; e += 256) {
      const int r = e / dv, v = e - r * dv;
      const int64_t row = blk + r;
      rb_f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
      if (row < q.end) x = *reinterpret_cast<const rb_f32x4*>(h + row * ldh + 4 * v);
      *reinterpret_cast<rb_f32x4*>(Hs + r * ldH + 4 * v) = x;
    }
    __syncthreads();
    const rb_f32x4 z = ss_scores(Hs + (wave * 16 + c) * ldH + 4 * g, ap, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t row = blk + wave * 16 + 4 * g + k;
      float p = 0.0f;
      if (row < q.end && oka) {
        const int64_t t = target[row];
        if (t >= 0 && t < V) {
          float zk = z[k] + shift;
          if constexpr (kItems) zk += isa;
          p = scale * expf(zk - lse[row]);
        }
      }
      Pt[(wave * 16 + 4 * g + k) * kPtLd + c] = p;
    }
    __syncthreads();
    // A = P^T [column c][row 4 g + k], B = H [row 4 g + k][16 dt + c]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int dt = wave + 4 * i;
      if (dt < DT) {
        for (int tt = 0; tt < 4; ++tt) {
          if (blk + tt * 16 >= q.end) break;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int r = tt * 16 + 4 * g + k;
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(Pt[r * kPtLd + c],
                                                          Hs[r * ldH + dt * 16 + c], acc[i], 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int dt = wave + 4 * i;
    if (dt >= DT) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int col = nt * 16 + 4 * g + k;
      if (col < n) dneg[(q.b * n + col) * d + dt * 16 + c] = acc[i][k];
    }
  }
}

int ss_row_blocks(int64_t max_len) {
  const int64_t rb = (max_len + kSsRows - 1) / kSsRows;
  return (int)(rb < 1 ? 1 : rb > kSsMaxBlocks ? kSsMaxBlocks : rb);
}

}  // namespace

int64_t shared_softmax_blocks(int64_t B, int64_t max_len) { return B * ss_row_blocks(max_len); }

int64_t shared_softmax_workspace_bytes(int64_t B, int64_t max_len) {
  return LossTailWs::bytes(shared_softmax_blocks(B, max_len));
}

int launch_shared_softmax_fwd(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                              const int64_t* neg, const int64_t* offsets, const int64_t* order,
                              int64_t M, int64_t B, int64_t d, int64_t V, int64_t n,
                              int64_t max_len, float shift, const float* item_shift, float* lse,
                              float* z0, float* loss, int64_t* n_live, void* workspace,
                              hipStream_t st) {
  const char* fn = item_shift ? "rb_shared_softmax_fwd_items" : "rb_shared_softmax_fwd";
  const int RB = ss_row_blocks(max_len);
  const int64_t nb = B * RB;
  const LossTailWs ws(workspace, nb);
  if (!ws.reset(st)) return launch_status(fn);
  hipLaunchKernelGGL(item_shift ? k_ss_fwd<true> : k_ss_fwd<false>, dim3((unsigned)nb), dim3(256),
                     0, st, h, ldh, tab, target, neg, offsets, order, M, B, (int)d, V, (int)n, RB,
                     shift, item_shift, lse, z0, ws.psum, ws.pcnt, ws.ticket, loss, n_live);
  return launch_status(fn);
}

int launch_shared_softmax_bwd(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                              const int64_t* neg, const int64_t* offsets, const int64_t* order,
                              const float* lse, const float* dloss, const int64_t* n_live,
                              int64_t M, int64_t B, int64_t d, int64_t V, int64_t n,
                              int64_t max_len, float shift, const float* item_shift, float* dh,
                              float* coef, float* dneg, hipStream_t st) {
  const char* fn = item_shift ? "rb_shared_softmax_bwd_items" : "rb_shared_softmax_bwd";
  const int RB = ss_row_blocks(max_len);
  hipLaunchKernelGGL(item_shift ? k_ss_dh<true> : k_ss_dh<false>, dim3((unsigned)(B * RB)),
                     dim3(256), 0, st, h, ldh, tab, target, neg, offsets, order, lse, dloss,
                     n_live, M, B, (int)d, V, (int)n, RB, shift, item_shift, dh, coef);
  if (int rc = launch_status(fn)) return rc;
  const int64_t NT = (n + 15) / 16;
  const size_t lds = (size_t)kSsRows * (d + 4 + kPtLd) * sizeof(float);
  hipLaunchKernelGGL(item_shift ? k_ss_dneg<true> : k_ss_dneg<false>, dim3((unsigned)(B * NT)),
                     dim3(256), lds, st, h, ldh, tab, target, neg, offsets, order, lse, dloss,
                     n_live, M, B, (int)d, V, (int)n, shift, item_shift, dneg);
  return launch_status(fn);
}

}  // namespace rb

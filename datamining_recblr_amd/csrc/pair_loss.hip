// pair_loss.hip — the sampled pairwise (BPR) loss of all-position training:
// per-position negative sampling on the device and the loss over each row's
// target and its sampled negatives only (include/recblr_pairs.h).
//
//   rb_sample_negatives   one workgroup per batch row: the row's seen set
//                         (its window's items and its target) sits in LDS,
//                         every (position, negative) draw is one thread that
//                         rejects Philox candidates against it;
//   rb_sample_negatives_alias  the same kernel body with the candidates drawn
//                         from an alias table instead of uniformly.  Attempt a
//                         = 0 .. 15 takes the words (u, v) = (2 (a % 2), 2 (a %
//                         2) + 1) of philox(counter = (b, t, j, a / 2)): the bin
//                         is i = mulhi(u, R), its table word holds the
//                         threshold (low 32 bits) and the alias bin (high 32
//                         bits), the candidate is first + (v < threshold ? i :
//                         alias).  One 8-byte read-only load per attempt;
//   rb_pair_loss_fwd      x = h.E[pos] - h.E[neg], l = -log(gamma + sigmoid(x)),
//                         a 16-lane group per row (row_group.h: the scoring
//                         core the candidate kernels share), the mean over
//                         the live pairs by loss_tail.h;
//   rb_pair_loss_bwd      dh and the per-(row, id column) coefficients the
//                         table's gradient is applied with
//                         (rb_embedding_bwd_apply_scaled, embedding.hip).
// No float atomics: every sum has a fixed order.
#include "common.h"
#include "loss_tail.h"
#include "row_group.h"

namespace rb {
namespace {

constexpr int kAttempts = 16;        // rejection attempts before the walk
constexpr int kRowsPerGroup = 4;
constexpr int kRowsPerWg = kGroups * kRowsPerGroup;   // 64
constexpr float kLn2 = 0.6931471805599453f;

// ---- negative sampling ----------------------------------------------------------
// seen[0 .. ns): the row's ids (out-of-range ones stored as -1, which no
// candidate equals).  Every lane scans all of it: the loads are broadcasts
// and the loop is uniform across the wave.
__device__ __forceinline__ bool is_seen(const int* seen, int ns, uint32_t cand) {
  bool s = false;
  for (int i = 0; i < ns; ++i) s |= seen[i] == (int)cand;
  return s;
}

// the walk after 16 rejections: upward, cyclically, from the 16th candidate
__device__ __forceinline__ int64_t walk_negative(const int* seen, int ns, uint32_t cand,
                                                 uint32_t first, uint32_t R) {
  uint32_t off = cand - first;
  for (uint32_t k = 1; k < R; ++k) {
    off = off + 1 == R ? 0u : off + 1;
    if (!is_seen(seen, ns, first + off)) return (int64_t)(first + off);
  }
  return -1;   // every id of [first, V) is seen
}

// the negative of (b, t, j): attempt a is word a % 4 of philox(counter =
// (b, t, j, a / 4)); the first unseen candidate of 16 wins, then the walk
__device__ int64_t draw_negative(const int* seen, int ns, uint32_t b, uint32_t t, uint32_t j,
                                 uint32_t first, uint32_t R, uint32_t k0, uint32_t k1) {
  uint32_t cand = first;
  for (uint32_t g = 0; g < kAttempts / 4; ++g) {
    const uint4 r = philox4x32_10(make_uint4(b, t, j, g), k0, k1);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      cand = first + __umulhi(w[a], R);
      if (!is_seen(seen, ns, cand)) return (int64_t)cand;
    }
  }
  return walk_negative(seen, ns, cand, first, R);
}

// ... from the alias table [R]: attempt a is the words (2 (a % 2), 2 (a % 2) +
// 1) of philox(counter = (b, t, j, a / 2)).  An alias bin past the table is
// read as the last one, so a candidate never leaves [first, V).
__device__ int64_t draw_negative_alias(const int* seen, int ns, uint32_t b, uint32_t t, uint32_t j,
                                       uint32_t first, uint32_t R, uint32_t k0, uint32_t k1,
                                       const int64_t* __restrict__ alias) {
  uint32_t cand = first;
  for (uint32_t g = 0; g < kAttempts / 2; ++g) {
    const uint4 r = philox4x32_10(make_uint4(b, t, j, g), k0, k1);
    const uint32_t u[2] = {r.x, r.z}, v[2] = {r.y, r.w};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const uint32_t i = __umulhi(u[a], R);
      const uint64_t e = (uint64_t)alias[i];
      const uint32_t other = min((uint32_t)(e >> 32), R - 1);
      cand = first + (v[a] < (uint32_t)e ? i : other);
      if (!is_seen(seen, ns, cand)) return (int64_t)cand;
    }
  }
  return walk_negative(seen, ns, cand, first, R);
}

template <bool kAlias>
__global__ void __launch_bounds__(256)
k_sample_negatives(const int64_t* __restrict__ item_seq, int64_t seq_rs,
                   const int64_t* __restrict__ lengths, const int64_t* __restrict__ pos_items,
                   const int64_t* __restrict__ offsets, const int64_t* __restrict__ inv, int64_t B,
                   int64_t L, int n_neg, int64_t first, int64_t V, uint32_t k0, uint32_t k1,
                   int64_t ntok, int64_t m_pad, const int64_t* __restrict__ alias,
                   int64_t* __restrict__ neg) {
  extern __shared__ int seen[];   // L + 1 ids
  const int64_t b = blockIdx.x;
  if (b >= B) {   // the workgroups past the batch: the padding rows [ntok, m_pad)
    const int64_t i = (b - B) * 256 + threadIdx.x;
    if (i < (m_pad - ntok) * n_neg) neg[ntok * n_neg + i] = -1;
    return;
  }
  const int64_t len = min(max(lengths[b], (int64_t)1), L);
  const int64_t* row = item_seq + b * seq_rs;
  for (int64_t i = threadIdx.x; i < len; i += 256) {
    const int64_t v = row[i];
    seen[i] = (v >= 0 && v < V) ? (int)v : -1;
  }
  if (threadIdx.x == 0) {
    const int64_t v = pos_items[b];
    seen[len] = (v >= 0 && v < V) ? (int)v : -1;
  }
  __syncthreads();
  const int ns = (int)len + 1;
  const bool dense = offsets != nullptr;
  int64_t row0 = b, t0 = len - 1, nt = 1;   // last position only, into row b
  if (dense) {
    const int64_t s = inv[b];
    row0 = (s >= 0 && s < B) ? offsets[s] : -1;
    if (row0 < 0) return;   // a malformed plan writes nothing for this row
    t0 = 0;
    nt = len;
  }
  const int64_t rows = dense ? ntok : B;
  for (int64_t w = threadIdx.x; w < nt * n_neg; w += 256) {
    const int64_t t = t0 + w / n_neg, j = w % n_neg;
    const int64_t r = dense ? row0 + t : row0;
    if (r >= rows) continue;
    if constexpr (kAlias)
      neg[r * n_neg + j] = draw_negative_alias(seen, ns, (uint32_t)b, (uint32_t)t, (uint32_t)j,
                                               (uint32_t)first, (uint32_t)(V - first), k0, k1,
                                               alias);
    else
      neg[r * n_neg + j] = draw_negative(seen, ns, (uint32_t)b, (uint32_t)t, (uint32_t)j,
                                         (uint32_t)first, (uint32_t)(V - first), k0, k1);
  }
}

// ---- the loss ---------------------------------------------------------------------
// sigmoid(x) and 1 - sigmoid(x) without cancellation (x >= 0: e = exp(-x) <=
// 1 and 1 - s = e s; x < 0: s <= 1/2).  exp(-x) = inf gives s = 0 exactly.
__device__ __forceinline__ void sigm2(float x, float& s, float& oms) {
  const float e = fexp(-x);
  s = frcp(1.0f + e);
  oms = x >= 0.0f ? e * s : 1.0f - s;
}

// Rows r = 64 * workgroup + 16 * i + group.  Ids are clamped for the loads
// and the result masked, so the code is uniform across the wave (the
// shuffles of group_sum see every lane).
template <int NV4>
__global__ void __launch_bounds__(256)
k_pair_fwd(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
           const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, int64_t M, int d,
           int64_t V, int n_neg, float gamma, float* __restrict__ diff, float* psum, int* pcnt,
           unsigned* ticket, float* __restrict__ loss, int64_t* __restrict__ n_live) {
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  float sum = 0.0f;
  int cnt = 0;
  for (int i = 0; i < kRowsPerGroup; ++i) {
    const int64_t r = (int64_t)blockIdx.x * kRowsPerWg + i * kGroups + g;
    const bool in = r < M;
    const int64_t rc = in ? r : M - 1;
    const int64_t p = pos[rc];
    const bool row_live = in && p >= 0 && p < V;
    const bool row_bad = in && (p < -1 || p >= V);
    float4 hv[NV4], ep[NV4];
    load_row<NV4>(hv, h + rc * ldh, l, d);
    load_row<NV4>(ep, tab + (row_live ? p : 0) * d, l, d);
    const float sp = dot_rows<NV4>(hv, ep);
    for (int j = 0; j < n_neg; ++j) {
      const int64_t q = neg[rc * n_neg + j];
      const bool q_ok = q >= 0 && q < V;
      const bool bad = row_bad || (in && (q < -1 || q >= V));
      const bool live = row_live && q_ok;
      float4 eq[NV4];
      load_row<NV4>(eq, tab + (q_ok ? q : 0) * d, l, d);
      const float x = sp - dot_rows<NV4>(hv, eq);
      float s, oms;
      sigm2(x, s, oms);
      const float lp = -(__builtin_amdgcn_logf(gamma + s) * kLn2);
      sum += bad ? NAN : live ? lp : 0.0f;
      cnt += live ? 1 : 0;
      if (in && l == 0) diff[r * n_neg + j] = live ? x : 0.0f;
    }
  }
  mean_loss_tail<kGroups>(sum, cnt, psum, pcnt, ticket, loss, n_live);
}

template <int NV4>
__global__ void __launch_bounds__(256)
k_pair_bwd(const float* __restrict__ tab, const int64_t* __restrict__ pos,
           const int64_t* __restrict__ neg, const float* __restrict__ diff,
           const float* __restrict__ dloss, const int64_t* __restrict__ n_live, int64_t M, int d,
           int64_t V, int n_neg, float gamma, float* __restrict__ dh, float* __restrict__ coef) {
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  const int64_t n = n_live[0];
  const float scale = dloss[0] / (float)(n > 0 ? n : 1);
  // s (1 - s) / (gamma + s) = (1 - s) / (1 + gamma (1 + exp(-x))), the product
  // gamma exp(-x) taken as exp2(-x log2(e) + log2(gamma)): at x = -100, where s
  // = e^-100 is below fp32's range, it is still 2.7e33 and the coefficient
  // (-3.7e-34) keeps its fp32 accuracy; past exp(-x) gamma = inf it is 0
  const float lg = __builtin_amdgcn_logf(gamma);   // -inf for gamma = 0
  for (int i = 0; i < kRowsPerGroup; ++i) {
    const int64_t r = (int64_t)blockIdx.x * kRowsPerWg + i * kGroups + g;
    if (r >= M) continue;
    const int64_t p = pos[r];
    const bool row_live = p >= 0 && p < V;
    float4 ep[NV4], acc[NV4];
    load_row<NV4>(ep, tab + (row_live ? p : 0) * d, l, d);
#pragma unroll
    for (int k = 0; k < NV4; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    float csum = 0.0f;
    for (int j = 0; j < n_neg; ++j) {
      const int64_t q = neg[r * n_neg + j];
      const bool live = row_live && q >= 0 && q < V;
      float4 eq[NV4];
      load_row<NV4>(eq, tab + (live ? q : 0) * d, l, d);
      float s, oms;
      const float x = diff[r * n_neg + j];
      sigm2(x, s, oms);
      const float ge = gamma + __builtin_amdgcn_exp2f(-x * kLog2e + lg);
      const float c = live ? scale * (-oms * frcp(1.0f + ge)) : 0.0f;
#pragma unroll
      for (int k = 0; k < NV4; ++k) {
        acc[k].x += live ? c * (ep[k].x - eq[k].x) : 0.0f;
        acc[k].y += live ? c * (ep[k].y - eq[k].y) : 0.0f;
        acc[k].z += live ? c * (ep[k].z - eq[k].z) : 0.0f;
        acc[k].w += live ? c * (ep[k].w - eq[k].w) : 0.0f;
      }
      csum += c;
      if (l == 0) coef[(int64_t)(1 + j) * M + r] = live ? -c : 0.0f;
    }
    if (l == 0) coef[r] = csum;
#pragma unroll
    for (int k = 0; k < NV4; ++k) {
      const int col = 4 * (l + kGroup * k);
      if (col < d) *reinterpret_cast<float4*>(dh + r * d + col) = acc[k];
    }
  }
}

int64_t pair_blocks(int64_t M) { return (M + kRowsPerWg - 1) / kRowsPerWg; }

}  // namespace

int64_t pair_loss_workspace_bytes(int64_t M) { return LossTailWs::bytes(pair_blocks(M)); }

int launch_sample_negatives(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                            const int64_t* pos_items, const int64_t* offsets, const int64_t* inv,
                            int64_t B, int64_t L, int64_t n_neg, int64_t first, int64_t V,
                            uint64_t seed, int64_t ntok, int64_t m_pad, const int64_t* alias,
                            int64_t* neg, hipStream_t st) {
  const int64_t pad_blocks = ((m_pad - ntok) * n_neg + 255) / 256;
  const auto kernel = alias ? k_sample_negatives<true> : k_sample_negatives<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(B + pad_blocks)), dim3(256),
                     (size_t)(L + 1) * sizeof(int), st, item_seq, seq_rs, lengths, pos_items,
                     offsets, inv, B, L, (int)n_neg, first, V, (uint32_t)seed,
                     (uint32_t)(seed >> 32), ntok, m_pad, alias, neg);
  return launch_status(alias ? "rb_sample_negatives_alias" : "rb_sample_negatives");
}

int launch_pair_loss_fwd(const float* h, int64_t ldh, const float* tab, const int64_t* pos,
                         const int64_t* neg, int64_t M, int64_t d, int64_t V, int64_t n_neg,
                         float gamma, float* diff, float* loss, int64_t* n_live, void* workspace,
                         hipStream_t st) {
  const int64_t nb = pair_blocks(M);
  const LossTailWs ws(workspace, nb);
  if (!ws.reset(st)) return launch_status("rb_pair_loss_fwd");
  dispatch_row_vecs(d, [&](auto nv) {
    hipLaunchKernelGGL((k_pair_fwd<decltype(nv)::value>), dim3((unsigned)nb), dim3(256), 0, st, h,
                       ldh, tab, pos, neg, M, (int)d, V, (int)n_neg, gamma, diff, ws.psum, ws.pcnt,
                       ws.ticket, loss, n_live);
  });
  return launch_status("rb_pair_loss_fwd");
}

int launch_pair_loss_bwd(const float* tab, const int64_t* pos, const int64_t* neg,
                         const float* diff, const float* dloss, const int64_t* n_live, int64_t M,
                         int64_t d, int64_t V, int64_t n_neg, float gamma, float* dh, float* coef,
                         hipStream_t st) {
  const int64_t nb = pair_blocks(M);
  dispatch_row_vecs(d, [&](auto nv) {
    hipLaunchKernelGGL((k_pair_bwd<decltype(nv)::value>), dim3((unsigned)nb), dim3(256), 0, st, tab,
                       pos, neg, diff, dloss, n_live, M, (int)d, V, (int)n_neg, gamma, dh, coef);
  });
  return launch_status("rb_pair_loss_bwd");
}

}  // namespace rb

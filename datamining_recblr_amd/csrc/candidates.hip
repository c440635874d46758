// candidates.hip — scoring chosen items (include/recblr_candidates.h): each
// row of h against a list of candidate ids instead of the whole item table.
//
//   rb_candidate_scores   scores[b, c] = h_b . table[cand[b, c]], a grid over
//                         the flattened (row, candidate) pairs;
//   rb_candidate_topk     one workgroup per row: score, filter, order and
//                         write in one launch (a bitonic sort of 64-bit keys
//                         in LDS, duplicates dropped where they sit adjacent);
//   rb_candidate_ranks    per row, the listed entries scoring above / equal to
//                         the row's target (integer counts).
//
// One scoring core serves the three and the pairwise loss (row_group.h): a
// 16-lane group per (row, id), 16-B loads, the dot product reduced inside the
// group.  A pair's score is a pure function of h_b's and table[id]'s d
// floats: its bits do not depend on the id's place in the list, on B or C,
// or on the entry point, so two equal table rows tie exactly and the top-k's
// and the ranks' comparisons are the plain scores'.  No float atomics.
#include "common.h"
#include "row_group.h"

namespace rb {
namespace {

constexpr int kRankChunk = 1024;      // candidates per workgroup of the ranks kernel
constexpr unsigned long long kDropped = ~0ull;   // sorts behind every selectable key

// The score of (h row, table row id).  The caller passes an id inside [0, V)
// (clamped) and masks the result, so every lane of the wave takes part in the
// shuffles and nothing out of range is read.
template <int NV4>
__device__ __forceinline__ float score(const float4 (&hv)[NV4], const float* tab, int64_t id,
                                       int l, int d) {
  float4 e[NV4];
  load_row<NV4>(e, tab + id * d, l, d);
  return dot_rows<NV4>(hv, e);
}

// ---- scores -----------------------------------------------------------------------
// Pair p = (16 * per) * workgroup + 16 * i + group, i < per; b = p / C, c = p % C.
template <int NV4>
__global__ void __launch_bounds__(256)
k_cand_scores(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
              const int64_t* __restrict__ cand, int64_t n_pairs, int64_t C, int d, int64_t V,
              int per, float* __restrict__ out) {
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  for (int i = 0; i < per; ++i) {
    const int64_t p = ((int64_t)blockIdx.x * per + i) * kGroups + g;
    const bool in = p < n_pairs;
    const int64_t pc = in ? p : n_pairs - 1;
    const int64_t id = cand[pc];
    const bool ok = id >= 0 && id < V;
    float4 hv[NV4];
    load_row<NV4>(hv, h + (pc / C) * ldh, l, d);
    const float s = score<NV4>(hv, tab, ok ? id : 0, l, d);
    if (in && l == 0) out[p] = ok ? s : -INFINITY;
  }
}

// ---- top-k --------------------------------------------------------------------------
// fp32 -> uint32, increasing with the value (-0 taken as +0, so the two tie
// as they compare); and back
__device__ __forceinline__ uint32_t ordered_bits(float s) {
  const uint32_t u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_ordered_bits(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

// One workgroup per row.  LDS: keys [P] (P = C rounded up to a power of two),
// then the row's exclude list as int [E] (-1 for an entry outside [0, V)).
// A selectable candidate's key is (~ordered_bits(score), id): ascending keys
// are (score descending, id ascending); everything else is kDropped (a
// selectable key's high word is never all ones: that would be a NaN's bits).
template <int NV4>
__global__ void __launch_bounds__(256)
k_cand_topk(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
            const int64_t* __restrict__ cand, int C, int P, int d, int64_t V, int64_t first,
            int64_t k, const int64_t* __restrict__ exclude, int E, int64_t* __restrict__ ids,
            float* __restrict__ scores) {
  extern __shared__ unsigned long long keys[];
  int* excl = reinterpret_cast<int*>(keys + P);
  __shared__ int wave_total[256 / kWave];
  const int tid = threadIdx.x, g = tid / kGroup, l = tid % kGroup;
  const int64_t b = blockIdx.x;

  for (int e = tid; e < E; e += 256) {
    const int64_t v = exclude[b * E + e];
    excl[e] = (v >= 0 && v < V) ? (int)v : -1;
  }
  __syncthreads();

  float4 hv[NV4];
  load_row<NV4>(hv, h + b * ldh, l, d);
  const int c_end = (C + kGroups - 1) / kGroups * kGroups;
  for (int c0 = 0; c0 < c_end; c0 += kGroups) {
    const int c = c0 + g;
    const int64_t id = c < C ? cand[b * C + c] : -1;
    const bool ok = id >= first && id < V;
    const float s = score<NV4>(hv, tab, ok ? id : 0, l, d);
    const int me = ok ? (int)id : -2;   // -2: equals no entry of excl
    int hit = 0;
    for (int e = l; e < E; e += kGroup) hit |= excl[e] == me;
    hit = group_or(hit);
    if (l == 0 && c < P) {
      const bool sel = ok && !hit && s == s;
      keys[c] = sel ? ((unsigned long long)(~ordered_bits(s)) << 32) | (uint32_t)id : kDropped;
    }
  }
  for (int c = c_end + tid; c < P; c += 256) keys[c] = kDropped;
  __syncthreads();

  // bitonic sort, ascending
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += 256) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const unsigned long long a = keys[i], c = keys[i | j];
        if ((a > c) == ((i & kk) == 0)) {
          keys[i] = c;
          keys[i | j] = a;
        }
      }
      __syncthreads();
    }
  }

  // equal ids now sit next to each other (equal id, equal score, equal key):
  // a survivor is the first of its run.  Thread t owns positions [t * per, (t
  // + 1) * per); its survivors' ranks follow from a prefix sum over the counts.
  const int per = P >= 256 ? P / 256 : 1;
  const int i0 = tid * per, i1 = min(i0 + per, P);
  int cnt = 0;
  for (int i = i0; i < i1; ++i)
    cnt += keys[i] != kDropped && (i == 0 || keys[i] != keys[i - 1]);
  const int lane = tid % kWave, wave = tid / kWave;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  if (lane == kWave - 1) wave_total[wave] = incl;
  __syncthreads();
  int64_t r = incl - cnt, n = 0;
  for (int w = 0; w < 256 / kWave; ++w) {
    r += w < wave ? wave_total[w] : 0;
    n += wave_total[w];
  }
  for (int i = i0; i < i1; ++i) {
    const unsigned long long key = keys[i];
    if (key == kDropped || (i > 0 && key == keys[i - 1])) continue;
    if (r < k) {
      ids[b * k + r] = (int64_t)(uint32_t)key;
      scores[b * k + r] = from_ordered_bits(~(uint32_t)(key >> 32));
    }
    ++r;
  }
  for (int64_t t = n + tid; t < k; t += 256) {
    ids[b * k + t] = -1;
    scores[b * k + t] = -INFINITY;
  }
}

// ---- ranks --------------------------------------------------------------------------
// Workgroup (b, chunk): candidates [chunk * 1024, + 1024) of row b, a group per
// candidate; the chunk's two counts are added to the row's (integer adds: any
// order gives the same sums; the launcher zeroes them first).  A target outside
// [first, V): chunk 0 adds -1 to both and nothing else is added.
template <int NV4>
__global__ void __launch_bounds__(256)
k_cand_ranks(const float* __restrict__ h, int64_t ldh, const float* __restrict__ tab,
             const int64_t* __restrict__ target, const int64_t* __restrict__ cand, int64_t C,
             int chunks, int d, int64_t V, int64_t first, unsigned long long* n_gt,
             unsigned long long* n_eq) {
  __shared__ int s_gt[kGroups], s_eq[kGroups];
  const int g = threadIdx.x / kGroup, l = threadIdx.x % kGroup;
  const int64_t b = blockIdx.x / chunks, c_lo = (int64_t)(blockIdx.x % chunks) * kRankChunk;
  const int64_t c_hi = min(c_lo + kRankChunk, C);
  const int64_t tgt = target[b];
  const bool t_ok = tgt >= first && tgt < V;
  float4 hv[NV4];
  load_row<NV4>(hv, h + b * ldh, l, d);
  const float st = score<NV4>(hv, tab, t_ok ? tgt : 0, l, d);
  int gt = 0, eq = 0;
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += kGroups) {
    const int64_t c = c0 + g;
    const int64_t id = c < c_hi ? cand[b * C + c] : -1;
    const bool ok = id >= first && id < V && id != tgt;
    const float s = score<NV4>(hv, tab, ok ? id : 0, l, d);   // a NaN compares false twice
    gt += ok && s > st;
    eq += ok && s == st;
  }
  if (l == 0) {
    s_gt[g] = gt;
    s_eq[g] = eq;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long a = 0, e = 0;
    for (int i = 0; i < kGroups; ++i) {
      a += s_gt[i];
      e += s_eq[i];
    }
    if (!t_ok) a = e = c_lo == 0 ? -1 : 0;
    atomicAdd(n_gt + b, (unsigned long long)a);
    atomicAdd(n_eq + b, (unsigned long long)e);
  }
}

int pow2_at_least(int64_t n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace

int launch_candidate_scores(const float* h, int64_t ldh, const float* tab, const int64_t* cand,
                            int64_t B, int64_t C, int64_t d, int64_t V, float* scores,
                            hipStream_t st) {
  const int64_t n = B * C;
  // few pairs: one per group, so that a single row's list still spreads over the device
  const int per = n <= (int64_t)num_cus() * 4 * kGroups ? 1 : 4;
  const int64_t nb = (n + (int64_t)per * kGroups - 1) / ((int64_t)per * kGroups);
  dispatch_row_vecs(d, [&](auto nv) {
    hipLaunchKernelGGL((k_cand_scores<decltype(nv)::value>), dim3((unsigned)nb), dim3(256), 0, st,
                       h, ldh, tab, cand, n, C, (int)d, V, per, scores);
  });
  return launch_status("rb_candidate_scores");
}

int launch_candidate_topk(const float* h, int64_t ldh, const float* tab, const int64_t* cand,
                          int64_t B, int64_t C, int64_t d, int64_t V, int64_t first, int64_t k,
                          const int64_t* exclude, int64_t E, int64_t* ids, float* scores,
                          hipStream_t st) {
  const int P = pow2_at_least(C);
  const size_t lds = (size_t)P * 8 + (size_t)E * 4;   // <= 32 KB + 16 KB
  dispatch_row_vecs(d, [&](auto nv) {
    hipLaunchKernelGGL((k_cand_topk<decltype(nv)::value>), dim3((unsigned)B), dim3(256), lds, st,
                       h, ldh, tab, cand, (int)C, P, (int)d, V, first, k, exclude, (int)E, ids,
                       scores);
  });
  return launch_status("rb_candidate_topk");
}

int launch_candidate_ranks(const float* h, int64_t ldh, const float* tab, const int64_t* target,
                           const int64_t* cand, int64_t B, int64_t C, int64_t d, int64_t V,
                           int64_t first, int64_t* n_gt, int64_t* n_eq, hipStream_t st) {
  const int64_t chunks = (C + kRankChunk - 1) / kRankChunk;
  if (hipMemsetAsync(n_gt, 0, (size_t)B * 8, st) != hipSuccess ||
      hipMemsetAsync(n_eq, 0, (size_t)B * 8, st) != hipSuccess)
    return launch_status("rb_candidate_ranks");
  dispatch_row_vecs(d, [&](auto nv) {
    hipLaunchKernelGGL((k_cand_ranks<decltype(nv)::value>), dim3((unsigned)(B * chunks)),
                       dim3(256), 0, st, h, ldh, tab, target, cand, C, (int)chunks, (int)d, V,
                       first, reinterpret_cast<unsigned long long*>(n_gt),
                       reinterpret_cast<unsigned long long*>(n_eq));
  });
  return launch_status("rb_candidate_ranks");
}

int64_t candidate_rank_chunks(int64_t C) { return (C + kRankChunk - 1) / kRankChunk; }

}  // namespace rb

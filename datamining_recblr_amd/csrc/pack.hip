// pack.hip — the packed-sequence plan of RecBLR._forward_packed in one launch.
//
// RecBole right-pads every sequence of a batch to L (RecBLR.py:75 reads
// item_seq [B, L] and item_seq_len [B]); the encoder runs only each
// sequence's first len_b positions, packed back to back longest first
// (DESIGN.md §3).  Given the packed order and the row offsets, one wave per
// packed sequence writes
//   ids[r]  = item_seq[order[s], t]   (the packed item ids the embedding reads)
//   pos[r]  = t                       (row r's position inside its sequence)
//   inv[order[s]]  = s,  last[order[s]] = offs[s+1] - 1
// for r = offs[s] + t — what a dozen torch index/arange/scatter launches did.
#include "common.h"

namespace rb {
namespace {

__global__ void __launch_bounds__(256)
k_pack_plan(const int64_t* __restrict__ seq, int64_t seq_rs, const int64_t* __restrict__ offs,
            const int64_t* __restrict__ order, int64_t B, int64_t* __restrict__ ids,
            int64_t* __restrict__ pos, int64_t* __restrict__ inv, int64_t* __restrict__ last) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= B) return;   // wave-uniform
  const int lane = threadIdx.x & 63;
  const int64_t b = order[s];
  const int64_t r0 = offs[s];
  const int64_t len = offs[s + 1] - r0;
  const int64_t* src = seq + b * seq_rs;
  for (int64_t t = lane; t < len; t += 64) {
    ids[r0 + t] = src[t];
    pos[r0 + t] = t;
  }
  if (lane == 0) {
    inv[b] = s;
    last[b] = r0 + len - 1;
  }
}

// The all-position training targets of the packed rows (RecBLR.forward_all:
// row r of packed sequence s holds the representation of the prefix sample
// items[:t+1] -> items[t+1]): one thread per row r < m_pad finds its sequence
// by bisection of offs (every probe inside [0, B]) and writes
//   tgt[r] = ids[r + 1]            r + 1 inside the same sequence
//          = pos_items[order[s]]   r the sequence's last row
//          = -1                    r >= ntok (the CE's padding rows), or
//                                  offs / order out of range for r.
// Every row is written exactly once; plain stores.
__global__ void __launch_bounds__(256)
k_next_item_targets(const int64_t* __restrict__ ids, const int64_t* __restrict__ offs,
                    const int64_t* __restrict__ order, const int64_t* __restrict__ pos_items,
                    int64_t B, int64_t ntok, int64_t m_pad, int64_t* __restrict__ tgt) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= m_pad) return;
  int64_t out = -1;
  if (r < ntok) {
    int64_t lo = 0, hi = B;   // offs[lo] <= r < offs[hi] for a well-formed plan
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (offs[mid] <= r) lo = mid; else hi = mid;
    }
    const int64_t r0 = offs[lo], r1 = offs[lo + 1];
    if (r0 <= r && r < r1 && r1 <= ntok) {
      if (r + 1 < r1) {
        out = ids[r + 1];
      } else {
        const int64_t b = order[lo];
        if (b >= 0 && b < B) out = pos_items[b];
      }
    }
  }
  tgt[r] = out;
}

}  // namespace

int launch_next_item_targets(const int64_t* ids, const int64_t* offs, const int64_t* order,
                             const int64_t* pos_items, int64_t B, int64_t ntok, int64_t m_pad,
                             int64_t* tgt, hipStream_t st) {
  const int64_t blocks = (m_pad + 255) / 256;
  hipLaunchKernelGGL(k_next_item_targets, dim3((unsigned)blocks), dim3(256), 0, st, ids, offs,
                     order, pos_items, B, ntok, m_pad, tgt);
  return launch_status("rb_next_item_targets");
}

int launch_pack_plan(const int64_t* seq, int64_t seq_rs, const int64_t* offs,
                     const int64_t* order, int64_t B, int64_t* ids, int64_t* pos, int64_t* inv,
                     int64_t* last, hipStream_t st) {
  const int64_t blocks = (B + 3) / 4;
  hipLaunchKernelGGL(k_pack_plan, dim3((unsigned)blocks), dim3(256), 0, st, seq, seq_rs, offs,
                     order, B, ids, pos, inv, last);
  return launch_status("rb_pack_plan");
}

}  // namespace rb

// loss_tail.h — the mean over the live terms of a loss kernel (k_pair_fwd,
// k_ss_fwd): per-workgroup partials that the last workgroup to arrive adds in
// workgroup order.  No float atomics: the sum has a fixed order.
#pragma once

#include "common.h"

namespace rb {

// The workspace of a launch of nb workgroups: the ticket in its own 16-B
// block, then float psum[nb], then int pcnt[nb].
struct LossTailWs {
  unsigned* ticket;
  float* psum;
  int* pcnt;

  static int64_t bytes(int64_t nb) { return 16 + nb * 8; }
  LossTailWs(void* base, int64_t nb)
      : ticket(static_cast<unsigned*>(base)),
        psum(reinterpret_cast<float*>(static_cast<char*>(base) + 16)),
        pcnt(reinterpret_cast<int*>(psum + nb)) {}
  // before every launch: the ticket counts from 0
  bool reset(hipStream_t st) const { return hipMemsetAsync(ticket, 0, 16, st) == hipSuccess; }
};

// Called by all 256 threads of every workgroup.  Slot i is threads [i * 256 /
// kSlots, (i + 1) * 256 / kSlots); its first thread's (sum, cnt) is the slot's.
// Thread 0 adds the slots in order into the workgroup's partial; the last
// workgroup to take a ticket re-reads every partial (thread t: t, t + 256 ...),
// adds them in a 256-wide tree (float sums, 64-bit counts), writes loss = sum /
// max(n, 1) and n_live = n, and leaves the ticket at 0.
template <int kSlots>
__device__ __forceinline__ void mean_loss_tail(float sum, int cnt, float* psum, int* pcnt,
                                               unsigned* ticket, float* loss, int64_t* n_live) {
  constexpr int kLanes = 256 / kSlots;
  __shared__ float s_sum[kSlots];
  __shared__ int s_cnt[kSlots];
  __shared__ float red[256];
  __shared__ long long redc[256];
  __shared__ bool last;
  if (threadIdx.x % kLanes == 0) {
    s_sum[threadIdx.x / kLanes] = sum;
    s_cnt[threadIdx.x / kLanes] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.0f;
    int c = 0;
    for (int k = 0; k < kSlots; ++k) {
      a += s_sum[k];
      c += s_cnt[k];
    }
    psum[blockIdx.x] = a;
    pcnt[blockIdx.x] = c;
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  float a = 0.0f;
  long long c = 0;
  for (unsigned k = threadIdx.x; k < gridDim.x; k += 256) {
    a += psum[k];
    c += pcnt[k];
  }
  red[threadIdx.x] = a;
  redc[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      redc[threadIdx.x] += redc[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long n = redc[0];
    loss[0] = red[0] / (float)(n > 0 ? n : 1);
    n_live[0] = n;
    *ticket = 0u;
  }
}

}  // namespace rb

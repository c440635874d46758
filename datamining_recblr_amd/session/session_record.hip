// session_record.hip — the per-slot ring of the last S item ids a session has
// consumed (recblr_session.h: rb_session_record).
//
// The encoder kernels keep a slot's fixed-size state and forget its items;
// this kernel writes the ids they are about to consume into ring [N, S] at
// (count + j) % S, and hands the caller the slot's whole ring as it stands
// afterwards (seen [B, S]: the exclusion list of a recommendation).  It
// restates the encoder kernels' masking rule from items, slots, N and V alone
// and runs before them on the same stream, while count still holds the
// position of the call's first event.
//
// Layout: a wave owns one call row.  Lanes take 64 consecutive columns, so a
// 16-lane group is one RB_SESSION_TILE-column chunk: the group's bits of one
// ballot give the chunk's first 0, those of a second whether any event before
// it lies outside [0, V), and a popcount of the event ballot below the lane
// numbers the events.  Two passes over the row: the first counts the events
// (n), the second stores the last min(n, S) of them, each ring entry at most
// once, so no result rests on the order of two stores to one address.  seen
// takes the same ids at the same positions and, for the positions this call
// leaves alone, the old ring values: those entries are not written by the
// launch, so nothing it stores is read back.  Plain 8-byte vector loads and
// stores; no LDS, no atomics, no scratch.
#include "../csrc/common.h"
#include "recblr_session.h"

namespace rb {

namespace {

static_assert(kWave % RB_SESSION_TILE == 0, "a wave's columns are whole chunks");

// The events among the wave's 64 columns base + lane of call row `row`:
// returns the ballot of the lanes that hold a recorded event and the lane's
// id in v.  Columns at or past W count as the 0 padding.
__device__ __forceinline__ unsigned long long chunk_events(const int64_t* __restrict__ row,
                                                           int64_t base, int64_t W, int64_t V,
                                                           int lane, int64_t& v) {
  const int64_t c = base + lane;
  v = c < W ? row[c] : 0;
  const int g = lane / RB_SESSION_TILE, r = lane % RB_SESSION_TILE;
  constexpr unsigned kGroup = (1u << RB_SESSION_TILE) - 1;
  const unsigned zeros = (unsigned)(__ballot(v == 0) >> (g * RB_SESSION_TILE)) & kGroup;
  const int first0 = zeros ? __builtin_ctz(zeros) : RB_SESSION_TILE;
  const bool live = r < first0;                       // before the chunk's first 0
  const unsigned bad =
      (unsigned)(__ballot(live && (v < 0 || v >= V)) >> (g * RB_SESSION_TILE)) & kGroup;
  return __ballot(live && bad == 0);                  // a bad id masks its whole chunk
}

__global__ void __launch_bounds__(256)
k_session_record(const int64_t* __restrict__ items, int64_t B, int64_t W,
                 const int64_t* __restrict__ slots, const int64_t* __restrict__ count,
                 int64_t* __restrict__ ring, int64_t* __restrict__ seen, int64_t N, int S,
                 int64_t V) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;   // wave-uniform, as every branch on slot, n and W below
  const int64_t slot = slots ? slots[b] : b;
  int64_t* const seen_row = seen ? seen + b * S : nullptr;
  if (slot < 0 || slot >= N) {   // before any address is formed from it
    if (seen_row)
      for (int p = lane; p < S; p += kWave) seen_row[p] = -1;
    return;
  }
  const int64_t* const row = items + b * W;   // dereferenced for columns < W only
  int64_t* const ring_row = ring + slot * S;

  // pass 1: the number of events the encoder launches will consume
  int64_t n = 0;
  for (int64_t base = 0; base < W; base += kWave) {
    int64_t v;
    n += __popcll(chunk_events(row, base, W, V, lane, v));
  }
  // the ring position of event 0; count is never negative, a stray one must
  // not form an address
  int64_t cnt = count[slot] % S;
  if (cnt < 0) cnt += S;
  const int64_t skip = n > S ? n - S : 0;   // events older than the last S

  // pass 2: event j -> ring[(count + j) % S], for the last min(n, S) events
  int64_t j0 = 0;
  for (int64_t base = 0; base < W && n > 0; base += kWave) {
    int64_t v;
    const unsigned long long ev = chunk_events(row, base, W, V, lane, v);
    const int64_t j = j0 + __popcll(ev & ((1ull << lane) - 1));
    if (((ev >> lane) & 1) && j >= skip) {
      const int p = (int)((cnt + j) % S);
      ring_row[p] = v;
      if (seen_row) seen_row[p] = v;
    }
    j0 += __popcll(ev);
  }
  // the positions the call left alone: (p - count) mod S >= n
  if (seen_row && n < S) {
    for (int p = lane; p < S; p += kWave) {
      int64_t off = p - cnt;
      if (off < 0) off += S;
      if (off >= n) seen_row[p] = ring_row[p];
    }
  }
}

}  // namespace

int launch_session_record(const int64_t* items, int64_t B, int64_t W, const int64_t* slots,
                          const int64_t* count, int64_t* ring, int64_t* seen, int64_t N, int S,
                          int64_t V, hipStream_t st) {
  const int64_t blocks = (B + 3) / 4;   // one wave per call row, four per workgroup
  hipLaunchKernelGGL(k_session_record, dim3((unsigned)blocks), dim3(256), 0, st, items, B, W,
                     slots, count, ring, seen, N, S, V);
  return launch_status("rb_session_record");
}

}  // namespace rb

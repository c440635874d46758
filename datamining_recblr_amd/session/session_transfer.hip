// session_transfer.hip — park, resume and exchange session slots
// (recblr_session.h: rb_session_transfer, and the blob format it documents).
//
// A slot's state is scattered over 2 * layers + 3 tensors; a parked session
// is one row of words.  This kernel moves B slots between the two forms in
// one launch, either way or both ways at once, bit for bit.
//
// Layout: one workgroup of 256 threads per call row.  A row is 12 words
// (d = H = 4, one layer, no ring) to a few thousand (2,580 at d = 128,
// H = 256, K = 4, two layers, S = 200), so a workgroup covers it in at most a
// few 16-byte sweeps and B = 1 still has four waves of loads in flight; a
// wave per row would walk the same row in four times as many dependent
// sweeps.  The float parts (out, and per layer h and the conv history) start
// at word 4 and have lengths that are multiples of 4 words, so thread t moves
// the 16-byte pieces t, t + 256, ... of each part.  The ring moves as 8-byte
// entries: its rows in the state are only 8-byte aligned when S is odd.
// Thread 0 moves the header (tag, 0, count) and writes the status.
//
// Order within a row: the slot is range-checked first (a bad slot writes its
// zero row and leaves, the whole workgroup together).  With blob_in the row is
// then judged as a whole before anything is stored to the slot: every thread
// reads the header (one address), the threads share the ring entries, each
// wave ballots, and the four ballots meet in LDS across one barrier.  The
// verdict is the same in every thread of the workgroup, so every branch on
// it, as on the slot, is wave-uniform.  Then each piece is moved by one
// thread: it loads the old value, stores it to blob_out, and only then stores
// the new value (from blob_in, or the reset value with release) to the same
// place.  Nothing the launch stores is read back, no location is stored
// twice, no atomics, no scratch; the blobs carry the nontemporal hint (each
// is touched once), the state keeps the default policy (the step reads it
// next).
#include "../csrc/common.h"
#include "recblr_session.h"

namespace rb {

namespace {

constexpr int kThreads = 256;

struct TransferArgs {
  float* h[RB_SESSION_MAX_LAYERS];
  float* conv[RB_SESSION_MAX_LAYERS];
  const float* h0[RB_SESSION_MAX_LAYERS];
  int64_t* count;
  float* out;
  int64_t* ring;
  const int64_t* slots;
  const int32_t* blob_in;
  int32_t* blob_out;
  int32_t* status;
  int64_t B, N, V, S, row_words;
  int tag, release, n_layers, d, H, hist;   // hist = (K - 1) H words, 0 without a conv history
};

enum Fill { kKeep, kBlob, kZero, kH0 };

// One float part of n words (n % 4 == 0): p the slot's row in the state, in /
// outb the part's place in the blob rows (null when that blob is absent),
// fill what the slot receives: nothing, blob_in's words, zeros, or h0.
__device__ __forceinline__ void move_floats(float* __restrict__ p, int n,
                                            const int32_t* __restrict__ in,
                                            int32_t* __restrict__ outb, int fill,
                                            const float* __restrict__ h0) {
  rb_u32x4* const p4 = reinterpret_cast<rb_u32x4*>(p);
  const rb_u32x4* const in4 = reinterpret_cast<const rb_u32x4*>(in);
  rb_u32x4* const out4 = reinterpret_cast<rb_u32x4*>(outb);
  const rb_u32x4* const h04 = reinterpret_cast<const rb_u32x4*>(h0);
  for (int i = threadIdx.x; i < n / 4; i += kThreads) {
    if (outb) st_pol<kNT>(p4[i], out4 + i);          // the old value, before the new one
    if (fill == kBlob) p4[i] = ld_pol<kNT>(in4 + i);
    else if (fill == kH0) p4[i] = h04[i];
    else if (fill == kZero) p4[i] = rb_u32x4{0u, 0u, 0u, 0u};
  }
}

__global__ void __launch_bounds__(kThreads) k_session_transfer(const TransferArgs a) {
  __shared__ int s_bad[kThreads / kWave];
  const int tid = threadIdx.x;
  // one workgroup per call row: every branch below is workgroup-uniform
  const int64_t b = blockIdx.x;
  const int64_t slot = a.slots ? a.slots[b] : b;
  const int32_t* const in = a.blob_in ? a.blob_in + b * a.row_words : nullptr;
  int32_t* const outb = a.blob_out ? a.blob_out + b * a.row_words : nullptr;

  if (slot < 0 || slot >= a.N) {   // before any address is formed from it
    if (outb)
      for (int64_t i = tid; i < a.row_words / 4; i += kThreads)
        st_pol<kNT>(rb_u32x4{0u, 0u, 0u, 0u}, reinterpret_cast<rb_u32x4*>(outb) + i);
    if (a.status && tid == 0) a.status[b] = RB_SESSION_BAD_SLOT;
    return;
  }

  const int64_t ring_off = 4 + a.d + (int64_t)a.n_layers * (a.H + a.hist);   // words
  const int64_t* const ring_in = in ? reinterpret_cast<const int64_t*>(in + ring_off) : nullptr;

  // the verdict on blob_in's row, before the first store to the slot
  bool apply = false;
  int64_t count_in = 0;
  if (in) {
    const rb_u32x4 hd = ld_pol<kNT>(reinterpret_cast<const rb_u32x4*>(in));   // one address
    count_in = (int64_t)(((uint64_t)hd[3] << 32) | hd[2]);
    bool bad = (int32_t)hd[0] != a.tag || count_in < 0;
    if (a.S > 0) {
      for (int64_t i = tid; i < a.S; i += kThreads) {
        const int64_t v = ld_pol<kNT>(ring_in + i);
        bad |= v < -1 || v >= a.V;
      }
      const bool wave_bad = __ballot(bad) != 0;
      if ((tid & (kWave - 1)) == 0) s_bad[tid / kWave] = wave_bad;
      __syncthreads();
      bad = false;
#pragma unroll
      for (int w = 0; w < kThreads / kWave; ++w) bad |= s_bad[w] != 0;
    }
    apply = !bad;
  }
  const bool reset = a.release != 0;   // never together with blob_in

  // header: tag, 0, count
  if (tid == 0) {
    const int64_t old = a.count[slot];
    if (outb)
      st_pol<kNT>(rb_u32x4{(uint32_t)a.tag, 0u, (uint32_t)(uint64_t)old,
                           (uint32_t)((uint64_t)old >> 32)},
                  reinterpret_cast<rb_u32x4*>(outb));
    if (apply) a.count[slot] = count_in;
    else if (reset) a.count[slot] = 0;
    if (a.status) a.status[b] = in && !apply ? RB_SESSION_BAD_BLOB : RB_SESSION_MOVED;
  }

  // the float parts, in blob order
  const int fill = apply ? kBlob : reset ? kZero : kKeep;
  int64_t w = 4;
  move_floats(a.out + slot * a.d, a.d, in ? in + w : nullptr, outb ? outb + w : nullptr, fill,
              nullptr);
  w += a.d;
  for (int li = 0; li < a.n_layers; ++li) {
    move_floats(a.h[li] + slot * a.H, a.H, in ? in + w : nullptr, outb ? outb + w : nullptr,
                fill == kZero && a.h0[li] ? kH0 : fill, a.h0[li]);
    w += a.H;
    if (a.hist) {
      move_floats(a.conv[li] + slot * a.hist, a.hist, in ? in + w : nullptr,
                  outb ? outb + w : nullptr, fill, nullptr);
      w += a.hist;
    }
  }

  // the ring, 8 bytes an entry, and the row's zero pad (one entry when S is odd)
  if (a.S > 0) {
    int64_t* const ring_row = a.ring + slot * a.S;
    int64_t* const ring_out = outb ? reinterpret_cast<int64_t*>(outb + ring_off) : nullptr;
    for (int64_t i = tid; i < a.S; i += kThreads) {
      if (ring_out) st_pol<kNT>(ring_row[i], ring_out + i);
      if (apply) ring_row[i] = ld_pol<kNT>(ring_in + i);
      else if (reset) ring_row[i] = -1;
    }
    if (ring_out && (a.S & 1) && tid == 0) st_pol<kNT>((int64_t)0, ring_out + a.S);
  }
}

}  // namespace

int64_t session_blob_words(int64_t d, int64_t H, int64_t K, int64_t n_layers, int64_t S,
                           bool has_conv) {
  const int64_t hist = has_conv ? (K - 1) * H : 0;
  return (4 + d + n_layers * (H + hist) + 2 * S + 3) / 4 * 4;
}

int launch_session_transfer(const rb_session_layer* layers, int n_layers, int64_t* count,
                            float* out, int64_t* ring, const int64_t* slots,
                            const int32_t* blob_in, int32_t* blob_out, int32_t* status, int tag,
                            int release, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                            int64_t S, bool has_conv, int64_t row_words, hipStream_t st) {
  TransferArgs a{};
  for (int i = 0; i < n_layers; ++i) {
    a.h[i] = layers[i].h;
    a.conv[i] = layers[i].conv_state;
    a.h0[i] = layers[i].h0;
  }
  a.count = count; a.out = out; a.ring = ring; a.slots = slots;
  a.blob_in = blob_in; a.blob_out = blob_out; a.status = status;
  a.B = B; a.N = N; a.V = V; a.S = S; a.row_words = row_words;
  a.tag = tag; a.release = release; a.n_layers = n_layers; a.d = d; a.H = H;
  a.hist = has_conv ? (K - 1) * H : 0;
  hipLaunchKernelGGL(k_session_transfer, dim3((unsigned)B), dim3(kThreads), 0, st, a);
  return launch_status("rb_session_transfer");
}

}  // namespace rb

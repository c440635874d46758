// session_capi.hip — the extern "C" entry points of the session library
// (recblr_session.h): argument checks, then the launchers in session_step.hip,
// session_append.hip, session_capture.hip, session_record.hip and
// session_transfer.hip.
// Built with hidden visibility, so its error helpers (rb::fail,
// rb::launch_status) are its own and never interpose the product library's.
#include "../csrc/common.h"
#include "recblr_session.h"

#include <string>

namespace rb {

namespace {
thread_local std::string g_session_error;
}

int fail(const char* msg) {
  g_session_error = msg;
  return RB_EINVAL;
}

int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_session_error = std::string(what) + ": " + hipGetErrorString(e);
    return static_cast<int>(e);
  }
  return 0;
}

int64_t session_lds_bytes(int64_t d, int64_t H);
int launch_session_step(const rb_session_layer* layers, int n_layers, const float* emb,
                        const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                        const int64_t* slots, int64_t* count, float* out, float* y,
                        int32_t* status, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                        bool use_conv, bool use_ffn, hipStream_t st);
int launch_session_append(const rb_session_layer* layers, int n_layers, const float* emb,
                          const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                          const int64_t* slots, int64_t* count, float* out, float* y,
                          float* y_all, int32_t* status, int64_t B, int T, int64_t N, int64_t V,
                          int d, int H, int K, bool use_conv, bool use_ffn, hipStream_t st);
int launch_session_capture(const float* u, int64_t u_rs, const float* xc, int64_t xc_rs,
                           const float* rg, int64_t rg_rs, const float* lam, const float* gate_b,
                           const float* carries, const int64_t* offs, const int64_t* slots,
                           float* h, float* conv_state, int64_t B, int L, int64_t N, int H, int K,
                           hipStream_t st);
int launch_session_record(const int64_t* items, int64_t B, int64_t W, const int64_t* slots,
                          const int64_t* count, int64_t* ring, int64_t* seen, int64_t N, int S,
                          int64_t V, hipStream_t st);
int64_t session_blob_words(int64_t d, int64_t H, int64_t K, int64_t n_layers, int64_t S,
                           bool has_conv);
int launch_session_transfer(const rb_session_layer* layers, int n_layers, int64_t* count,
                            float* out, int64_t* ring, const int64_t* slots,
                            const int32_t* blob_in, int32_t* blob_out, int32_t* status, int tag,
                            int release, int64_t B, int64_t N, int64_t V, int d, int H, int K,
                            int64_t S, bool has_conv, int64_t row_words, hipStream_t st);
}  // namespace rb

using namespace rb;

extern "C" {

#define RB_EXPORT __attribute__((visibility("default")))

// the product library's rb_version() it pairs with
RB_EXPORT int rb_session_version(void) { return RB_ABI_VERSION; }

RB_EXPORT const char* rb_session_last_error_string(void) { return g_session_error.c_str(); }

RB_EXPORT int64_t rb_session_lds_bytes(int64_t d, int64_t H) {
  if (d <= 0 || H <= 0 || d > (1 << 20) || H > (1 << 20)) return RB_EINVAL;
  return session_lds_bytes(d, H);
}

// The checks rb_session_step and rb_session_append share; `who` prefixes the
// message ("rb_session_step: ").
static int check_encoder_args(const std::string& who, const rb_session_layer* layers,
                              int64_t n_layers, const float* emb, const float* ln_w,
                              const float* ln_b, float eps, const int64_t* items,
                              const int64_t* count, const float* out, const float* y, int64_t B,
                              int64_t N, int64_t V, int64_t d, int64_t H, int64_t K,
                              bool use_conv, bool use_ffn) {
  const auto no = [&](const char* what) { return fail((who + what).c_str()); };
  if (!layers || !emb || !ln_w || !ln_b || !items || !count || !out) return no("null pointer");
  if (n_layers < 1 || n_layers > RB_SESSION_MAX_LAYERS) return no("n_layers must be in [1, 8]");
  if (K < 1 || K > 8) return no("conv kernel size K must be in [1, 8]");
  if (d <= 0 || H <= 0 || d % 16 || H % 16 || d > (1 << 20) || H > (1 << 20))
    return no("d and H must be positive multiples of 16");
  if (B <= 0 || N <= 0 || V <= 0) return no("B, N and V must be positive");
  if (B >= (1LL << 31) || N >= (1LL << 31) || V >= (1LL << 31))
    return no("B, N and V must be < 2^31");
  if (session_lds_bytes(d, H) > RB_SESSION_MAX_LDS)
    return no("shape needs more LDS than a compute unit has (160 KiB)");
  if (!(eps > 0.0f)) return no("eps must be positive");
  // every operand the MFMA streams is read 16 bytes per lane
  if (!aligned16(emb) || !aligned16(out) || (y && !aligned16(y)))
    return no("emb, out and y must be 16-byte aligned");
  for (int64_t i = 0; i < n_layers; ++i) {
    const rb_session_layer& L = layers[i];
    if (!L.w_in || !L.w_gate || !L.b_gate || !L.lam || !L.w_out || !L.ln_w || !L.ln_b || !L.h)
      return no("null pointer in a layer");
    if (use_conv && (!L.conv_w || !L.conv_b || (K > 1 && !L.conv_state)))
      return no("null conv pointer in a layer");
    if (use_ffn && (!L.w1 || !L.b1 || !L.w2 || !L.b2 || !L.ffn_ln_w || !L.ffn_ln_b))
      return no("null ffn pointer in a layer");
    if (!aligned16(L.w_in) || !aligned16(L.w_gate) || !aligned16(L.w_out) ||
        (use_ffn && (!aligned16(L.w1) || !aligned16(L.w2))))
      return no("weight matrices must be 16-byte aligned");
  }
  return 0;
}

RB_EXPORT int rb_session_step(const rb_session_layer* layers, int64_t n_layers, const float* emb,
                    const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                    const int64_t* slots, int64_t* count, float* out, float* y,
                    int32_t* status, int64_t B, int64_t N, int64_t V, int64_t d, int64_t H,
                    int64_t K, int disable_conv1d, int disable_ffn, void* stream) {
  const bool use_conv = !disable_conv1d, use_ffn = !disable_ffn;
  if (int rc = check_encoder_args("rb_session_step: ", layers, n_layers, emb, ln_w, ln_b, eps,
                                  items, count, out, y, B, N, V, d, H, K, use_conv, use_ffn))
    return rc;
  return launch_session_step(layers, (int)n_layers, emb, ln_w, ln_b, eps, items, slots, count,
                             out, y, status, B, N, V, (int)d, (int)H, (int)K, use_conv, use_ffn,
                             reinterpret_cast<hipStream_t>(stream));
}

RB_EXPORT int rb_session_append(const rb_session_layer* layers, int64_t n_layers, const float* emb,
                      const float* ln_w, const float* ln_b, float eps, const int64_t* items,
                      const int64_t* slots, int64_t* count, float* out, float* y, float* y_all,
                      int32_t* status, int64_t B, int64_t T, int64_t N, int64_t V, int64_t d,
                      int64_t H, int64_t K, int disable_conv1d, int disable_ffn, void* stream) {
  const bool use_conv = !disable_conv1d, use_ffn = !disable_ffn;
  if (int rc = check_encoder_args("rb_session_append: ", layers, n_layers, emb, ln_w, ln_b, eps,
                                  items, count, out, y, B, N, V, d, H, K, use_conv, use_ffn))
    return rc;
  if (T != 1 && T != 2 && T != 4 && T != 8 && T != 16)
    return fail("rb_session_append: T must be 1, 2, 4, 8 or 16");
  if (y_all && !aligned16(y_all))
    return fail("rb_session_append: y_all must be 16-byte aligned");
  return launch_session_append(layers, (int)n_layers, emb, ln_w, ln_b, eps, items, slots, count,
                               out, y, y_all, status, B, (int)T, N, V, (int)d, (int)H, (int)K,
                               use_conv, use_ffn, reinterpret_cast<hipStream_t>(stream));
}

RB_EXPORT int rb_session_capture(const float* u, int64_t u_rs, const float* xc, int64_t xc_rs,
                       const float* rg, int64_t rg_rs, const float* lam, const float* gate_b,
                       const float* carries, const int64_t* seq_offsets, const int64_t* slots,
                       float* h, float* conv_state, int64_t B, int64_t L, int64_t N, int64_t H,
                       int64_t K, void* stream) {
  if (!u || !xc || !rg || !lam || !gate_b || !carries || !seq_offsets || !slots || !h)
    return fail("rb_session_capture: null pointer");
  if (K < 1 || K > 8) return fail("rb_session_capture: conv kernel size K must be in [1, 8]");
  if (H <= 0 || H % 4 || H > (1 << 20))
    return fail("rb_session_capture: H must be a positive multiple of 4");
  if (B <= 0 || L <= 0 || N <= 0) return fail("rb_session_capture: B, L and N must be positive");
  if (B >= (1LL << 31) || L >= (1LL << 31) || N >= (1LL << 31))
    return fail("rb_session_capture: B, L and N must be < 2^31");
  // one wave per (sequence, 256 channels), four waves per workgroup
  if (B * ((H + 255) / 256) >= (1LL << 26))
    return fail("rb_session_capture: too many (sequence, channel span) pairs for one launch");
  if (u_rs < H || xc_rs < H || rg_rs < 2 * H || u_rs % 4 || xc_rs % 4 || rg_rs % 4)
    return fail("rb_session_capture: row strides must be multiples of 4, at least H (rg: 2H)");
  if (!conv_state && K > 1 && xc != u)
    return fail("rb_session_capture: conv_state may be NULL only when K == 1 or xc == u");
  // every row piece is one 16-byte access per lane
  if (!aligned16(u) || !aligned16(xc) || !aligned16(rg) || !aligned16(lam) ||
      !aligned16(gate_b) || !aligned16(carries) || !aligned16(h) || !aligned16(conv_state))
    return fail("rb_session_capture: u, xc, rg, lam, gate_b, carries, h and conv_state must be "
                "16-byte aligned");
  return launch_session_capture(u, u_rs, xc, xc_rs, rg, rg_rs, lam, gate_b, carries, seq_offsets,
                                slots, h, conv_state, B, (int)L, N, (int)H, (int)K,
                                reinterpret_cast<hipStream_t>(stream));
}

RB_EXPORT int rb_session_record(const int64_t* items, int64_t B, int64_t W, const int64_t* slots,
                      const int64_t* count, int64_t* ring, int64_t* seen, int64_t N, int64_t S,
                      int64_t V, void* stream) {
  if (W < 0) return fail("rb_session_record: W must be >= 0");
  if ((!items && W > 0) || !count || !ring) return fail("rb_session_record: null pointer");
  if (B <= 0 || N <= 0 || S <= 0 || V <= 0)
    return fail("rb_session_record: B, N, S and V must be positive");
  if (B >= (1LL << 31) || N >= (1LL << 31) || S >= (1LL << 31) || V >= (1LL << 31) ||
      W >= (1LL << 31))
    return fail("rb_session_record: B, W, N, S and V must be < 2^31");
  return launch_session_record(items, B, W, slots, count, ring, seen, N, (int)S, V,
                               reinterpret_cast<hipStream_t>(stream));
}

// whether (d, H, K, n_layers, S) is a shape rb_session_blob_words sizes
static bool blob_shape_ok(int64_t d, int64_t H, int64_t K, int64_t n_layers, int64_t S) {
  return d > 0 && H > 0 && d <= (1 << 20) && H <= (1 << 20) && K >= 1 && K <= 8 &&
         n_layers >= 1 && n_layers <= RB_SESSION_MAX_LAYERS && S >= 0 && S < (1LL << 31);
}

RB_EXPORT int64_t rb_session_blob_words(int64_t d, int64_t H, int64_t K, int64_t n_layers,
                                        int64_t S, int has_conv) {
  if (!blob_shape_ok(d, H, K, n_layers, S)) return RB_EINVAL;
  return session_blob_words(d, H, K, n_layers, S, has_conv != 0);
}

RB_EXPORT int rb_session_transfer(const rb_session_layer* layers, int64_t n_layers, int64_t* count,
                        float* out, int64_t* ring, const int64_t* slots,
                        const int32_t* blob_in, int32_t* blob_out, int32_t* status,
                        int tag, int release, int64_t B, int64_t N, int64_t V, int64_t d,
                        int64_t H, int64_t K, int64_t S, int has_conv, int64_t row_words,
                        void* stream) {
  if (!layers || !count || !out) return fail("rb_session_transfer: null pointer");
  if (!blob_in && !blob_out && !release)
    return fail("rb_session_transfer: nothing to do: give blob_in, blob_out or release");
  if (blob_in && release)
    return fail("rb_session_transfer: release cannot be combined with blob_in");
  if (n_layers < 1 || n_layers > RB_SESSION_MAX_LAYERS)
    return fail("rb_session_transfer: n_layers must be in [1, 8]");
  if (K < 1 || K > 8) return fail("rb_session_transfer: conv kernel size K must be in [1, 8]");
  if (d <= 0 || H <= 0 || d % 4 || H % 4 || d > (1 << 20) || H > (1 << 20))
    return fail("rb_session_transfer: d and H must be positive multiples of 4");
  if (B <= 0 || N <= 0 || V <= 0) return fail("rb_session_transfer: B, N and V must be positive");
  if (S < 0) return fail("rb_session_transfer: S must be >= 0");
  if (B >= (1LL << 31) || N >= (1LL << 31) || V >= (1LL << 31) || S >= (1LL << 31))
    return fail("rb_session_transfer: B, N, V and S must be < 2^31");
  if (S > 0 && !ring) return fail("rb_session_transfer: null ring with S > 0");
  if (row_words != session_blob_words(d, H, K, n_layers, S, has_conv != 0))
    return fail("rb_session_transfer: row_words is not rb_session_blob_words of this shape");
  const bool hist = has_conv && K > 1;
  for (int64_t i = 0; i < n_layers; ++i) {
    const rb_session_layer& L = layers[i];
    if (!L.h || (hist && !L.conv_state))
      return fail("rb_session_transfer: null state pointer in a layer");
    if (!aligned16(L.h) || !aligned16(L.conv_state) || !aligned16(L.h0))
      return fail("rb_session_transfer: h, conv_state and h0 must be 16-byte aligned");
  }
  // the float parts and the blob rows move 16 bytes per lane
  if (!aligned16(out) || !aligned16(blob_in) || !aligned16(blob_out))
    return fail("rb_session_transfer: out, blob_in and blob_out must be 16-byte aligned");
  if (blob_in && blob_out) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(blob_in);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(blob_out);
    const uintptr_t bytes = (uintptr_t)B * (uintptr_t)row_words * 4;
    if (i0 < o0 + bytes && o0 < i0 + bytes)
      return fail("rb_session_transfer: blob_in and blob_out overlap");
  }
  return launch_session_transfer(layers, (int)n_layers, count, out, ring, slots, blob_in,
                                 blob_out, status, tag, release, B, N, V, (int)d, (int)H, (int)K,
                                 S, has_conv != 0, row_words,
                                 reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"

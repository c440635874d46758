// capi.hip — the extern "C" boundary declared in include/recblr_hip.h:
// argument validation, error reporting, dispatch to the kernel launchers.
#include "common.h"

#include <atomic>

namespace rb {

namespace {
thread_local std::string g_last_error;
}

int fail(const char* msg) {
  g_last_error = msg;
  return RB_EINVAL;
}

// an argument error of entry point fn: "<fn>: <msg>"
static int fail(const char* fn, const char* msg) {
  g_last_error = std::string(fn) + ": " + msg;
  return RB_EINVAL;
}

int num_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n <= 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

int launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return static_cast<int>(e);
  }
  return 0;
}

namespace {

// Per-lane offsets inside one batch row are 32-bit: L * row_stride must fit.
int check_dims(int64_t B, int64_t L, int64_t H, int64_t max_rs) {
  if (B <= 0 || L <= 0 || H <= 0) return fail("B, L and H must be positive");
  if (L * max_rs + max_rs >= (int64_t(1) << 31)) return fail("L * row_stride exceeds 2^31");
  if (B * ((H + 15) / 16) / 4 + 1 > 0x7fffffffLL) return fail("grid too large");
  return 0;
}

int64_t max4(int64_t a, int64_t b, int64_t c = 0, int64_t d = 0) {
  return std::max(std::max(a, b), std::max(c, d));
}

hipStream_t as_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }

// ---- the recurrence entry points: one body per operation, shared by the fp32
// (T = float) and bf16 (T = bf16_t) storage forms; fn is the entry point's name

template <typename T>
int scan_fwd(const char* fn, const T* gates, const T* tokens, T* states, int64_t B, int64_t C,
             int64_t steps, void* stream) {
  if (!gates || !tokens || !states) return fail(fn, "null pointer");
  if (B <= 0 || C <= 0 || steps <= 0) return fail(fn, "B, C, T must be positive");
  const int64_t rows = B * C;
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(fn, "too many rows");
  return launch_scan_fwd<T>(gates, tokens, states, rows, steps, as_stream(stream));
}

template <typename T>
int scan_bwd(const char* fn, const T* gates, const T* states, const T* grad, T* d_gates,
             T* d_tokens, int64_t B, int64_t C, int64_t steps, void* stream) {
  if (!gates || !states || !grad || !d_gates || !d_tokens) return fail(fn, "null pointer");
  if (B <= 0 || C <= 0 || steps <= 0) return fail(fn, "B, C, T must be positive");
  const int64_t rows = B * C;
  if ((rows + 3) / 4 > 0x7fffffffLL) return fail(fn, "too many rows");
  return launch_scan_bwd<T>(gates, states, grad, d_gates, d_tokens, rows, steps,
                            as_stream(stream));
}

template <typename T>
int conv_silu_fwd(const char* fn, const T* x, int64_t x_rs, const float* w, const float* bias,
                  T* xc, int64_t xc_rs, int64_t B, int64_t L, int64_t H, int64_t K,
                  const int64_t* seq_offsets, void* stream) {
  if (!x || !w || !bias || !xc) return fail(fn, "null pointer");
  if (K < 1 || K > 8) return fail(fn, "kernel size K must be in [1, 8]");
  if (x_rs < H || xc_rs < H) return fail(fn, "row stride < H");
  if (int r = check_dims(B, L, H, max4(x_rs, xc_rs))) return r;
  return launch_conv_fwd<T>(x, x_rs, w, bias, xc, xc_rs, B, L, H, K, seq_offsets,
                            as_stream(stream));
}

template <typename T>
int conv_silu_fwd_rows(const char* fn, const T* x, int64_t x_rs, const float* w,
                       const float* bias, T* xc, int64_t xc_rs, int64_t ntok, int64_t H,
                       int64_t K, const int64_t* row_pos, void* stream) {
  if (!x || !w || !bias || !xc || !row_pos) return fail(fn, "null pointer");
  if (K < 1 || K > 8) return fail(fn, "kernel size K must be in [1, 8]");
  if (x_rs < H || xc_rs < H) return fail(fn, "row stride < H");
  if (int r = check_dims(ntok, 1, H, max4(x_rs, xc_rs))) return r;
  return launch_conv_fwd_rows<T>(x, x_rs, w, bias, xc, xc_rs, ntok, H, K, row_pos,
                                 as_stream(stream));
}

template <typename T>
int conv_silu_bwd(const char* fn, const T* x, int64_t x_rs, const float* w, const float* bias,
                  const T* g1, const T* g2, T* dx, int64_t dx_rs, float* dw_part, float* db_part,
                  int64_t B, int64_t L, int64_t H, int64_t K, const int64_t* seq_offsets,
                  void* stream) {
  if (!x || !w || !bias || !g1 || !dx || !dw_part)   // db_part NULL: folded layout
    return fail(fn, "null pointer");
  if (K < 1 || K > 8) return fail(fn, "kernel size K must be in [1, 8]");
  if (x_rs < H || dx_rs < H) return fail(fn, "row stride < H");
  if (int r = check_dims(B, L, H, max4(x_rs, dx_rs, H))) return r;
  return launch_conv_bwd<T>(x, x_rs, w, bias, g1, g2, dx, dx_rs, dw_part, db_part, B, L, H, K,
                            seq_offsets, as_stream(stream));
}

// y_last / batch_row: rb_gate_scan_fwd_last (y NULL, y_rs = H); NULL otherwise.
// z_last: its sparse-z mode (z NULL, z_rs = H)
template <typename T>
int gate_scan_fwd(const char* fn, const T* rg, int64_t rg_rs, const T* xc, int64_t xc_rs,
                  const T* z, int64_t z_rs, const float* lam, const float* gate_b,
                  const float* h0, int64_t h0_bs, T* y, int64_t y_rs, float* carries, int64_t B,
                  int64_t L, int64_t H, const int64_t* seq_offsets, void* stream,
                  T* y_last = nullptr, const int64_t* batch_row = nullptr,
                  const T* z_last = nullptr) {
  if (!rg || !xc || !(z || z_last) || !lam || !(y || y_last)) return fail(fn, "null pointer");
  if (z && z_last) return fail(fn, "give z or z_last, not both");
  if (h0_bs != 0 && h0_bs < H) return fail(fn, "h0 batch stride must be 0 or >= H");
  if (rg_rs < 2 * H || xc_rs < H || z_rs < H || y_rs < H) return fail(fn, "row stride too small");
  if (int r = check_dims(B, L, H, max4(rg_rs, xc_rs, z_rs, y_rs))) return r;
  return launch_gate_fwd<T>(rg, rg_rs, xc, xc_rs, z, z_rs, lam, gate_b, h0, h0_bs, y, y_rs,
                            carries, B, L, H, seq_offsets, as_stream(stream), y_last, batch_row,
                            z_last);
}

// dy_last / batch_row: rb_gate_scan_bwd_last (dy NULL); NULL otherwise.
// z_last / dz_last: its sparse-z mode (z, dz NULL, z_rs = dz_rs = H)
template <typename T>
int gate_scan_bwd(const char* fn, const T* rg, int64_t rg_rs, const T* xc, int64_t xc_rs,
                  const T* z, int64_t z_rs, const float* lam, const float* gate_b,
                  const float* carries, const T* dy, T* drg, int64_t drg_rs, T* dxc,
                  int64_t dxc_rs, T* dz, int64_t dz_rs, float* part, float* dh0_part, int64_t B,
                  int64_t L, int64_t H, const int64_t* seq_offsets, void* stream,
                  const T* dy_last = nullptr, const int64_t* batch_row = nullptr,
                  const T* z_last = nullptr, T* dz_last = nullptr) {
  if (!rg || !xc || !(z || z_last) || !lam || !carries || !(dy || dy_last) || !drg || !dxc ||
      !(dz || dz_last) || !part || !dh0_part)
    return fail(fn, "null pointer");
  if ((z_last != nullptr) != (dz_last != nullptr) || (z && z_last) || (dz && dz_last))
    return fail(fn, "give z and dz, or z_last and dz_last");
  if (rg_rs < 2 * H || xc_rs < H || z_rs < H || drg_rs < 2 * H || dxc_rs < H || dz_rs < H)
    return fail(fn, "row stride too small");
  if (int r = check_dims(B, L, H, max4(max4(rg_rs, xc_rs, z_rs, drg_rs), dz_rs, dxc_rs, H)))
    return r;
  return launch_gate_bwd<T>(rg, rg_rs, xc, xc_rs, z, z_rs, lam, gate_b, carries, dy, drg, drg_rs,
                            dxc, dxc_rs, dz, dz_rs, part, dh0_part, B, L, H, seq_offsets,
                            as_stream(stream), dy_last, batch_row, z_last, dz_last);
}

// rb_bf16 (raw bits in the C header) is the kernels' bf16_t
const bf16_t* bf(const rb_bf16* p) { return reinterpret_cast<const bf16_t*>(p); }
bf16_t* bf(rb_bf16* p) { return reinterpret_cast<bf16_t*>(p); }

}  // namespace

DropSpec make_drop(const uint8_t* mask, uint64_t seed, float p) {
  DropSpec d{};
  d.mask = mask;
  d.scale = p > 0.0f ? 1.0f / (1.0f - p) : 1.0f;
  d.key0 = (uint32_t)seed;
  d.key1 = (uint32_t)(seed >> 32);
  const double keep = 1.0 - (double)p;
  d.keep_thresh = keep >= 1.0 ? 0xFFFFFFFFu : (uint32_t)(keep * 4294967296.0);
  d.mode = mask ? 1 : (p > 0.0f ? 2 : 0);
  return d;
}
}  // namespace rb

using namespace rb;

extern "C" {

int rb_version(void) { return RB_ABI_VERSION; }

const char* rb_last_error_string(void) { return g_last_error.c_str(); }

int rb_num_kernels(void) { return 24; }

int rb_scan_fwd(const float* gates, const float* tokens, float* states, int64_t B, int64_t C,
                int64_t T, void* stream) {
  return scan_fwd(__func__, gates, tokens, states, B, C, T, stream);
}

int rb_scan_bwd(const float* gates, const float* states, const float* grad, float* d_gates,
                float* d_tokens, int64_t B, int64_t C, int64_t T, void* stream) {
  return scan_bwd(__func__, gates, states, grad, d_gates, d_tokens, B, C, T, stream);
}

int rb_conv_silu_fwd(const float* x, int64_t x_rs, const float* w, const float* bias, float* xc,
                     int64_t xc_rs, int64_t B, int64_t L, int64_t H, int64_t K,
                     const int64_t* seq_offsets, void* stream) {
  return conv_silu_fwd(__func__, x, x_rs, w, bias, xc, xc_rs, B, L, H, K, seq_offsets, stream);
}

int rb_conv_silu_fwd_rows(const float* x, int64_t x_rs, const float* w, const float* bias,
                          float* xc, int64_t xc_rs, int64_t ntok, int64_t H, int64_t K,
                          const int64_t* row_pos, void* stream) {
  return conv_silu_fwd_rows(__func__, x, x_rs, w, bias, xc, xc_rs, ntok, H, K, row_pos, stream);
}

int rb_conv_silu_bwd(const float* x, int64_t x_rs, const float* w, const float* bias,
                     const float* g1, const float* g2, float* dx, int64_t dx_rs, float* dw_part,
                     float* db_part, int64_t B, int64_t L, int64_t H, int64_t K,
                     const int64_t* seq_offsets, void* stream) {
  return conv_silu_bwd(__func__, x, x_rs, w, bias, g1, g2, dx, dx_rs, dw_part, db_part, B, L, H,
                       K, seq_offsets, stream);
}

int rb_gate_scan_fwd(const float* rg, int64_t rg_rs, const float* xc, int64_t xc_rs,
                     const float* z, int64_t z_rs, const float* lam, const float* gate_b,
                     const float* h0, int64_t h0_bs, float* y, int64_t y_rs, float* carries,
                     int64_t B, int64_t L, int64_t H, const int64_t* seq_offsets, void* stream) {
  return gate_scan_fwd(__func__, rg, rg_rs, xc, xc_rs, z, z_rs, lam, gate_b, h0, h0_bs, y, y_rs,
                       carries, B, L, H, seq_offsets, stream);
}

int rb_gate_scan_bwd(const float* rg, int64_t rg_rs, const float* xc, int64_t xc_rs,
                     const float* z, int64_t z_rs, const float* lam, const float* gate_b,
                     const float* carries, const float* dy, float* drg, int64_t drg_rs,
                     float* dxc, int64_t dxc_rs, float* dz, int64_t dz_rs, float* part,
                     float* dh0_part, int64_t B, int64_t L, int64_t H,
                     const int64_t* seq_offsets, void* stream) {
  return gate_scan_bwd(__func__, rg, rg_rs, xc, xc_rs, z, z_rs, lam, gate_b, carries, dy, drg,
                       drg_rs, dxc, dxc_rs, dz, dz_rs, part, dh0_part, B, L, H, seq_offsets,
                       stream);
}

int rb_gate_scan_fwd_last(const float* rg, int64_t rg_rs, const float* xc, int64_t xc_rs,
                          const float* z, int64_t z_rs, const float* z_last, const float* lam,
                          const float* gate_b, const float* h0, int64_t h0_bs, float* y_last,
                          float* carries, int64_t B, int64_t L, int64_t H,
                          const int64_t* seq_offsets, const int64_t* batch_row, void* stream) {
  if (!y_last) return fail(__func__, "null pointer");
  return gate_scan_fwd<float>(__func__, rg, rg_rs, xc, xc_rs, z, z_last ? H : z_rs, lam, gate_b,
                              h0, h0_bs, nullptr, H, carries, B, L, H, seq_offsets, stream,
                              y_last, batch_row, z_last);
}

int rb_gate_scan_bwd_last(const float* rg, int64_t rg_rs, const float* xc, int64_t xc_rs,
                          const float* z, int64_t z_rs, const float* z_last, const float* lam,
                          const float* gate_b, const float* carries, const float* dy_last,
                          float* drg, int64_t drg_rs, float* dxc, int64_t dxc_rs, float* dz,
                          int64_t dz_rs, float* dz_last, float* part, float* dh0_part, int64_t B,
                          int64_t L, int64_t H, const int64_t* seq_offsets,
                          const int64_t* batch_row, void* stream) {
  if (!dy_last) return fail(__func__, "null pointer");
  return gate_scan_bwd<float>(__func__, rg, rg_rs, xc, xc_rs, z, z_last ? H : z_rs, lam, gate_b,
                              carries, nullptr, drg, drg_rs, dxc, dxc_rs, dz,
                              dz_last ? H : dz_rs, part, dh0_part, B, L, H, seq_offsets, stream,
                              dy_last, batch_row, z_last, dz_last);
}

// ---- bf16 storage variants (fp32 arithmetic; the same bodies as the fp32 forms) ----

int rb_scan_fwd_bf16(const rb_bf16* gates, const rb_bf16* tokens, rb_bf16* states, int64_t B,
                     int64_t C, int64_t T, void* stream) {
  return scan_fwd(__func__, bf(gates), bf(tokens), bf(states), B, C, T, stream);
}

int rb_scan_bwd_bf16(const rb_bf16* gates, const rb_bf16* states, const rb_bf16* grad,
                     rb_bf16* d_gates, rb_bf16* d_tokens, int64_t B, int64_t C, int64_t T,
                     void* stream) {
  return scan_bwd(__func__, bf(gates), bf(states), bf(grad), bf(d_gates), bf(d_tokens), B, C, T,
                  stream);
}

int rb_conv_silu_fwd_bf16(const rb_bf16* x, int64_t x_rs, const float* w, const float* bias,
                          rb_bf16* xc, int64_t xc_rs, int64_t B, int64_t L, int64_t H, int64_t K,
                          const int64_t* seq_offsets, void* stream) {
  return conv_silu_fwd(__func__, bf(x), x_rs, w, bias, bf(xc), xc_rs, B, L, H, K, seq_offsets,
                       stream);
}

int rb_conv_silu_fwd_rows_bf16(const rb_bf16* x, int64_t x_rs, const float* w, const float* bias,
                               rb_bf16* xc, int64_t xc_rs, int64_t ntok, int64_t H, int64_t K,
                               const int64_t* row_pos, void* stream) {
  return conv_silu_fwd_rows(__func__, bf(x), x_rs, w, bias, bf(xc), xc_rs, ntok, H, K, row_pos,
                            stream);
}

int rb_conv_silu_bwd_bf16(const rb_bf16* x, int64_t x_rs, const float* w, const float* bias,
                          const rb_bf16* g1, const rb_bf16* g2, rb_bf16* dx, int64_t dx_rs,
                          float* dw_part, float* db_part, int64_t B, int64_t L, int64_t H,
                          int64_t K, const int64_t* seq_offsets, void* stream) {
  return conv_silu_bwd(__func__, bf(x), x_rs, w, bias, bf(g1), bf(g2), bf(dx), dx_rs, dw_part,
                       db_part, B, L, H, K, seq_offsets, stream);
}

int rb_gate_scan_fwd_bf16(const rb_bf16* rg, int64_t rg_rs, const rb_bf16* xc, int64_t xc_rs,
                          const rb_bf16* z, int64_t z_rs, const float* lam, const float* gate_b,
                          const float* h0, int64_t h0_bs, rb_bf16* y, int64_t y_rs,
                          float* carries, int64_t B, int64_t L, int64_t H,
                          const int64_t* seq_offsets, void* stream) {
  return gate_scan_fwd(__func__, bf(rg), rg_rs, bf(xc), xc_rs, bf(z), z_rs, lam, gate_b, h0,
                       h0_bs, bf(y), y_rs, carries, B, L, H, seq_offsets, stream);
}

int rb_gate_scan_bwd_bf16(const rb_bf16* rg, int64_t rg_rs, const rb_bf16* xc, int64_t xc_rs,
                          const rb_bf16* z, int64_t z_rs, const float* lam, const float* gate_b,
                          const float* carries, const rb_bf16* dy, rb_bf16* drg, int64_t drg_rs,
                          rb_bf16* dxc, int64_t dxc_rs, rb_bf16* dz, int64_t dz_rs, float* part,
                          float* dh0_part, int64_t B, int64_t L, int64_t H,
                          const int64_t* seq_offsets, void* stream) {
  return gate_scan_bwd(__func__, bf(rg), rg_rs, bf(xc), xc_rs, bf(z), z_rs, lam, gate_b, carries,
                       bf(dy), bf(drg), drg_rs, bf(dxc), dxc_rs, bf(dz), dz_rs, part, dh0_part,
                       B, L, H, seq_offsets, stream);
}

int rb_add_ln_fwd(const float* a, const int64_t* idx, int64_t n_idx_rows, const uint8_t* mask,
                  uint64_t seed, float p, const float* r, const float* gamma, const float* beta,
                  float eps, float* y, float* s_out, float* mean, float* rstd, int64_t rows,
                  int64_t d, void* stream) {
  if (!a || !gamma || !beta || !y) return fail("rb_add_ln_fwd: null pointer");
  if (rows <= 0 || d <= 0) return fail("rb_add_ln_fwd: rows and d must be positive");
  if (idx && n_idx_rows <= 0) return fail("rb_add_ln_fwd: empty gather table");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_add_ln_fwd: dropout p must be in [0, 1)");
  if ((s_out == nullptr) != (mean == nullptr) || (mean == nullptr) != (rstd == nullptr))
    return fail("rb_add_ln_fwd: s_out, mean and rstd must be given together");
  return launch_add_ln_fwd(a, idx, n_idx_rows, make_drop(mask, seed, p), r, gamma, beta, eps, y,
                           s_out, mean, rstd, rows, d, reinterpret_cast<hipStream_t>(stream));
}

int64_t rb_row_num_parts(int64_t rows, int64_t width) {
  if (rows <= 0 || width <= 0) return 0;
  return ln_num_parts(rows, width);
}

int rb_add_ln_bwd2(const float* dy, const float* dy2, const float* s, const float* gamma,
                   const float* mean, const float* rstd, const uint8_t* mask, uint64_t seed,
                   float p, float* ds, float* da, float* dgamma_part, float* dbeta_part,
                   float* dbias_part, int64_t n_parts, int64_t rows, int64_t d, void* stream) {
  if (!dy || !s || !gamma || !mean || !rstd || !dgamma_part || !dbeta_part)
    return fail("rb_add_ln_bwd: null pointer");
  if (!ds && !da && !dbias_part) return fail("rb_add_ln_bwd: nothing to write");
  if (rows <= 0 || d <= 0) return fail("rb_add_ln_bwd: rows and d must be positive");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_add_ln_bwd: dropout p must be in [0, 1)");
  if (n_parts != ln_num_parts(rows, d)) return fail("rb_add_ln_bwd: n_parts != rb_row_num_parts");
  return launch_add_ln_bwd(dy, dy2, s, gamma, mean, rstd, make_drop(mask, seed, p), ds, da,
                           dgamma_part, dbeta_part, dbias_part, n_parts, rows, d,
                           reinterpret_cast<hipStream_t>(stream));
}

int rb_add_ln_bwd(const float* dy, const float* s, const float* gamma, const float* mean,
                  const float* rstd, const uint8_t* mask, uint64_t seed, float p, float* ds,
                  float* da, float* dgamma_part, float* dbeta_part, float* dbias_part,
                  int64_t n_parts, int64_t rows, int64_t d, void* stream) {
  return rb_add_ln_bwd2(dy, nullptr, s, gamma, mean, rstd, mask, seed, p, ds, da, dgamma_part,
                        dbeta_part, dbias_part, n_parts, rows, d, stream);
}

int rb_silu_dropout_fwd(const float* a, const float* bias, const uint8_t* mask, uint64_t seed,
                        float p, float* u, int64_t rows, int64_t cols, void* stream) {
  if (!a || !u) return fail("rb_silu_dropout_fwd: null pointer");
  if (bias && !aligned16(bias)) return fail("rb_silu_dropout_fwd: misaligned bias");
  if (rows <= 0 || cols <= 0) return fail("rb_silu_dropout_fwd: rows and cols must be positive");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_silu_dropout_fwd: dropout p must be in [0, 1)");
  if (!aligned16(a) || !aligned16(u) || (mask && (reinterpret_cast<uintptr_t>(mask) & 3)))
    return fail("rb_silu_dropout_fwd: misaligned buffer");
  return launch_silu_dropout_fwd(a, bias, make_drop(mask, seed, p), u, rows, cols,
                                 reinterpret_cast<hipStream_t>(stream));
}

int rb_silu_dropout_bwd(const float* a, const float* bias, const uint8_t* mask, uint64_t seed,
                        float p, const float* du, float* da, float* dbias_part, int64_t n_parts,
                        int64_t rows, int64_t cols, void* stream) {
  if (!a || !du || !da) return fail("rb_silu_dropout_bwd: null pointer");
  if (bias && !aligned16(bias)) return fail("rb_silu_dropout_bwd: misaligned bias");
  if (rows <= 0 || cols <= 0) return fail("rb_silu_dropout_bwd: rows and cols must be positive");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_silu_dropout_bwd: dropout p must be in [0, 1)");
  if (!aligned16(a) || !aligned16(du) || !aligned16(da) ||
      (mask && (reinterpret_cast<uintptr_t>(mask) & 3)))
    return fail("rb_silu_dropout_bwd: misaligned buffer");
  if (dbias_part && n_parts != ln_num_parts(rows, cols))
    return fail("rb_silu_dropout_bwd: n_parts != rb_row_num_parts");
  return launch_silu_dropout_bwd(a, bias, make_drop(mask, seed, p), du, da, dbias_part,
                                 ln_num_parts(rows, cols), rows, cols,
                                 reinterpret_cast<hipStream_t>(stream));
}

int rb_dropout_mask(uint64_t seed, float p, uint8_t* out, int64_t n, void* stream) {
  if (!out) return fail("rb_dropout_mask: null pointer");
  if (n <= 0 || n % 4) return fail("rb_dropout_mask: n must be a positive multiple of 4");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_dropout_mask: dropout p must be in [0, 1)");
  return launch_dropout_mask(make_drop(nullptr, seed, p), out, n,
                             reinterpret_cast<hipStream_t>(stream));
}

int64_t rb_embedding_bwd_workspace(int64_t M, int64_t V, int64_t d) {
  if (M <= 0 || V <= 0 || d <= 0) return 0;
  return emb_workspace_bytes(M, V, d);
}

int rb_embedding_bwd_plan(const int64_t* idx, int64_t M, int64_t d, int64_t V, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  if (!idx || !workspace) return fail("rb_embedding_bwd_plan: null pointer");
  if (M <= 0 || d <= 0 || V <= 0) return fail("rb_embedding_bwd_plan: M, d, V must be positive");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 30))
    return fail("rb_embedding_bwd_plan: M or V too large");
  return launch_embedding_plan(idx, M, d, V, workspace, workspace_bytes,
                               reinterpret_cast<hipStream_t>(stream));
}

int rb_embedding_bwd_apply(const float* grad, int64_t M, int64_t d, int64_t V,
                           int64_t padding_idx, float* dweight, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  if (!grad || !dweight || !workspace) return fail("rb_embedding_bwd_apply: null pointer");
  if (M <= 0 || d <= 0 || V <= 0) return fail("rb_embedding_bwd_apply: M, d, V must be positive");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 30))
    return fail("rb_embedding_bwd_apply: M or V too large");
  return launch_embedding_apply(grad, M, d, V, padding_idx, dweight, workspace, workspace_bytes,
                                reinterpret_cast<hipStream_t>(stream));
}

int rb_embedding_bwd(const int64_t* idx, const float* grad, int64_t M, int64_t d, int64_t V,
                     int64_t padding_idx, float* dweight, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  if (!idx || !grad || !dweight || !workspace) return fail("rb_embedding_bwd: null pointer");
  if (M <= 0 || d <= 0 || V <= 0) return fail("rb_embedding_bwd: M, d, V must be positive");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 30))
    return fail("rb_embedding_bwd: M or V too large");
  return launch_embedding_bwd(idx, grad, M, d, V, padding_idx, dweight, workspace,
                              workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

namespace {
int check_items(const char* fn, const float* seq, const float* items, int64_t B, int64_t V,
                int64_t d) {
  (void)fn;
  if (!seq || !items) return fail("item scores: null pointer");
  if (B <= 0 || V <= 0) return fail("item scores: B and V must be positive");
  if (d != 16 && d != 32 && d != 64 && d != 128 && d != 256)
    return fail("item scores: d must be 16, 32, 64, 128 or 256");
  if (!aligned16(seq) || !aligned16(items)) return fail("item scores: operands must be 16-B aligned");
  if (B >= (int64_t(1) << 31) || V >= (int64_t(1) << 31)) return fail("item scores: B or V too large");
  return 0;
}
}  // namespace

int64_t rb_item_ce_workspace(int64_t B, int64_t V, int64_t d) {
  if (B <= 0 || V <= 0 || d <= 0) return 0;
  return item_ce_workspace_bytes(B, V, d);
}

int rb_item_ce_fwd(const float* seq, const float* items, const int64_t* target, int64_t B,
                   int64_t V, int64_t d, float* lse, float* loss, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  if (int rc = check_items("rb_item_ce_fwd", seq, items, B, V, d)) return rc;
  if (!target || !lse || !loss || !workspace) return fail("rb_item_ce_fwd: null pointer");
  return launch_item_ce_fwd(seq, items, target, B, V, d, lse, loss, workspace, workspace_bytes,
                            reinterpret_cast<hipStream_t>(stream));
}

int rb_item_ce_bwd(const float* seq, const float* items, const int64_t* target, const float* lse,
                   const float* dloss, int64_t B, int64_t V, int64_t d, float* dseq,
                   float* ditems, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_items("rb_item_ce_bwd", seq, items, B, V, d)) return rc;
  if (!target || !lse || !dloss || !workspace) return fail("rb_item_ce_bwd: null pointer");
  return launch_item_ce_bwd(seq, items, target, lse, dloss, B, V, d, dseq, ditems, workspace,
                            workspace_bytes, reinterpret_cast<hipStream_t>(stream));
}

int64_t rb_item_rank_workspace(int64_t B, int64_t V, int64_t d) {
  if (B <= 0 || V <= 0 || d <= 0) return 0;
  return item_rank_workspace_bytes(B, V);
}

namespace {
// what rb_item_rank and rb_item_rank_allowed check alike
int check_item_rank(const char* fn, const float* seq, const float* items, const int64_t* target,
                    int64_t B, int64_t V, int64_t d, int64_t first_item,
                    const int64_t* n_greater, const void* workspace) {
  if (int rc = check_items(fn, seq, items, B, V, d)) return rc;
  if (!target || !n_greater || !workspace) return fail(fn, "null pointer");
  if (first_item < 0) return fail(fn, "first_item must be >= 0");
  return 0;
}

// ... and rb_item_topk and rb_item_topk_allowed
int check_item_topk(const char* fn, const float* seq, const float* items, int64_t B, int64_t V,
                    int64_t d, int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                    const int64_t* ids, const float* scores, const void* workspace) {
  if (int rc = check_items(fn, seq, items, B, V, d)) return rc;
  if (!ids || !scores || !workspace) return fail(fn, "null pointer");
  if (k < 1 || k > 64) return fail(fn, "k must be in [1, 64]");
  if (first_item < 0) return fail(fn, "first_item must be >= 0");
  if (E < 0) return fail(fn, "E must be >= 0");
  if (E > 0 && !exclude) return fail(fn, "null pointer (exclude with E > 0)");
  return 0;
}

// the allow-bitmaps of include/recblr_filters.h (after the checks above: V > 0)
int check_allow(const char* fn, const int32_t* allow, int64_t F, int64_t words, int64_t V) {
  if (!allow) return fail(fn, "null pointer (allow)");
  if (F < 1) return fail(fn, "F must be >= 1");
  if (words != (V + 31) / 32) return fail(fn, "words must be ceil(V / 32)");
  return 0;
}

// Every rb_item_rank* after its own required-argument rule: the shared checks,
// then each option that is present (allow, prior: non-null) checked and packed.
int item_rank(const char* fn, const float* seq, const float* items, const int64_t* target,
              int64_t B, int64_t V, int64_t d, int64_t first_item, int64_t* n_greater,
              int64_t* n_equal, void* workspace, int64_t workspace_bytes, void* stream,
              const int32_t* allow, int64_t F, int64_t words, const int64_t* allow_rows,
              const float* prior, int64_t P, const int64_t* prior_rows,
              const float* prior_weight) {
  if (int rc = check_item_rank(fn, seq, items, target, B, V, d, first_item, n_greater, workspace))
    return rc;
  if (allow)
    if (int rc = check_allow(fn, allow, F, words, V)) return rc;
  const AllowArgs al{allow, F, words, allow_rows};
  const PriorArgs pa{prior, P, V, prior_rows, prior_weight};
  return launch_item_rank(fn, seq, items, target, B, V, d, first_item, n_greater, n_equal,
                          workspace, workspace_bytes, allow ? &al : nullptr,
                          prior ? &pa : nullptr, reinterpret_cast<hipStream_t>(stream));
}

// ... and every rb_item_topk* (groups non-null: the cap)
int item_topk(const char* fn, const float* seq, const float* items, int64_t B, int64_t V,
              int64_t d, int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
              int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes, void* stream,
              const int32_t* allow, int64_t F, int64_t words, const int64_t* allow_rows,
              const int32_t* groups, int64_t max_per_group, const float* prior, int64_t P,
              const int64_t* prior_rows, const float* prior_weight) {
  if (int rc = check_item_topk(fn, seq, items, B, V, d, k, first_item, exclude, E, ids, scores,
                               workspace))
    return rc;
  if (allow)
    if (int rc = check_allow(fn, allow, F, words, V)) return rc;
  if (groups && max_per_group < 1) return fail(fn, "max_per_group must be >= 1");
  const AllowArgs al{allow, F, words, allow_rows};
  // a cap of k or more never binds: clamp it into the kernel's int
  const GroupArgs gr{groups, (int)std::min<int64_t>(max_per_group, k)};
  const PriorArgs pa{prior, P, V, prior_rows, prior_weight};
  return launch_item_topk(fn, seq, items, B, V, d, k, first_item, E > 0 ? exclude : nullptr, E,
                          ids, scores, workspace, workspace_bytes, allow ? &al : nullptr,
                          groups ? &gr : nullptr, prior ? &pa : nullptr,
                          reinterpret_cast<hipStream_t>(stream));
}
}  // namespace

int rb_item_rank(const float* seq, const float* items, const int64_t* target, int64_t B,
                 int64_t V, int64_t d, int64_t first_item, int64_t* n_greater, int64_t* n_equal,
                 void* workspace, int64_t workspace_bytes, void* stream) {
  return item_rank("rb_item_rank", seq, items, target, B, V, d, first_item, n_greater, n_equal,
                   workspace, workspace_bytes, stream, /*filter*/ nullptr, 0, 0, nullptr,
                   /*prior*/ nullptr, 0, nullptr, nullptr);
}

int rb_item_rank_allowed(const float* seq, const float* items, const int64_t* target, int64_t B,
                         int64_t V, int64_t d, int64_t first_item, int64_t* n_greater,
                         int64_t* n_equal, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows) {
  const char* fn = "rb_item_rank_allowed";
  if (!allow) return fail(fn, "null pointer (allow)");
  return item_rank(fn, seq, items, target, B, V, d, first_item, n_greater, n_equal, workspace,
                   workspace_bytes, stream, allow, F, words, allow_rows,
                   /*prior*/ nullptr, 0, nullptr, nullptr);
}

int64_t rb_item_topk_workspace(int64_t B, int64_t V, int64_t d, int64_t k) {
  if (B <= 0 || V <= 0 || d <= 0 || k < 1 || k > 64) return 0;
  return item_topk_workspace_bytes(B, V, k);
}

int rb_item_topk(const float* seq, const float* items, int64_t B, int64_t V, int64_t d, int64_t k,
                 int64_t first_item, const int64_t* exclude, int64_t E, int64_t* ids,
                 float* scores, void* workspace, int64_t workspace_bytes, void* stream) {
  return item_topk("rb_item_topk", seq, items, B, V, d, k, first_item, exclude, E, ids, scores,
                   workspace, workspace_bytes, stream, /*filter*/ nullptr, 0, 0, nullptr,
                   /*cap*/ nullptr, 0, /*prior*/ nullptr, 0, nullptr, nullptr);
}

int rb_item_topk_allowed(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                         int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                         int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows) {
  const char* fn = "rb_item_topk_allowed";
  if (!allow) return fail(fn, "null pointer (allow)");
  return item_topk(fn, seq, items, B, V, d, k, first_item, exclude, E, ids, scores, workspace,
                   workspace_bytes, stream, allow, F, words, allow_rows, /*cap*/ nullptr, 0,
                   /*prior*/ nullptr, 0, nullptr, nullptr);
}

int64_t rb_item_topk_grouped_workspace(int64_t B, int64_t V, int64_t d, int64_t k) {
  if (B <= 0 || V <= 0 || d <= 0 || k < 1 || k > 64) return 0;
  return item_topk_grouped_workspace_bytes(B, V, k);
}

int rb_item_topk_grouped(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                         int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                         int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                         void* stream, const int32_t* allow, int64_t F, int64_t words,
                         const int64_t* allow_rows, const int32_t* groups,
                         int64_t max_per_group) {
  const char* fn = "rb_item_topk_grouped";
  if (!groups) return fail(fn, "null pointer (groups)");
  return item_topk(fn, seq, items, B, V, d, k, first_item, exclude, E, ids, scores, workspace,
                   workspace_bytes, stream, allow, F, words, allow_rows, groups, max_per_group,
                   /*prior*/ nullptr, 0, nullptr, nullptr);
}

int64_t rb_item_topk_prior_workspace(int64_t B, int64_t V, int64_t d, int64_t k) {
  if (B <= 0 || V <= 0 || d <= 0 || k < 1 || k > 64) return 0;
  return item_topk_grouped_workspace_bytes(B, V, k);
}

int rb_item_topk_prior(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                       int64_t k, int64_t first_item, const int64_t* exclude, int64_t E,
                       int64_t* ids, float* scores, void* workspace, int64_t workspace_bytes,
                       void* stream, const int32_t* allow, int64_t F, int64_t words,
                       const int64_t* allow_rows, const int32_t* groups, int64_t max_per_group,
                       const float* prior, int64_t P, const int64_t* prior_rows,
                       const float* prior_weight) {
  const char* fn = "rb_item_topk_prior";
  if (!prior) return fail(fn, "null pointer (prior)");
  if (P < 1) return fail(fn, "P must be >= 1");
  return item_topk(fn, seq, items, B, V, d, k, first_item, exclude, E, ids, scores, workspace,
                   workspace_bytes, stream, allow, F, words, allow_rows, groups, max_per_group,
                   prior, P, prior_rows, prior_weight);
}

int rb_item_rank_prior(const float* seq, const float* items, const int64_t* target, int64_t B,
                       int64_t V, int64_t d, int64_t first_item, int64_t* n_greater,
                       int64_t* n_equal, void* workspace, int64_t workspace_bytes, void* stream,
                       const int32_t* allow, int64_t F, int64_t words, const int64_t* allow_rows,
                       const float* prior, int64_t P, const int64_t* prior_rows,
                       const float* prior_weight) {
  const char* fn = "rb_item_rank_prior";
  if (!prior) return fail(fn, "null pointer (prior)");
  if (P < 1) return fail(fn, "P must be >= 1");
  return item_rank(fn, seq, items, target, B, V, d, first_item, n_greater, n_equal, workspace,
                   workspace_bytes, stream, allow, F, words, allow_rows, prior, P, prior_rows,
                   prior_weight);
}

int rb_item_ce_probs(const float* seq, const float* items, const int64_t* target,
                     const float* lse, const float* dloss, int64_t B, int64_t V, int64_t d,
                     int64_t item_offset, float* probs, int64_t ld, void* stream) {
  if (int rc = check_items("rb_item_ce_probs", seq, items, B, V, d)) return rc;
  if (!target || !lse || !dloss || !probs) return fail("rb_item_ce_probs: null pointer");
  if (ld < V) return fail("rb_item_ce_probs: ld < V");
  return launch_item_ce_probs(seq, items, target, lse, dloss, B, V, d, item_offset, probs, ld,
                              reinterpret_cast<hipStream_t>(stream));
}

int rb_item_split_h(const float* x, int64_t n, int64_t d, void* image, int* exps,
                    float* group_max, void* stream) {
  if (!x || !image || !exps) return fail("rb_item_split_h: null pointer");
  if (n <= 0) return fail("rb_item_split_h: n must be positive");
  if (d != 16 && d != 32 && d != 64 && d != 128 && d != 256)
    return fail("rb_item_split_h: d must be 16, 32, 64, 128 or 256");
  if (!aligned16(x) || !aligned16(image)) return fail("rb_item_split_h: operands must be 16-B aligned");
  if (n >= (int64_t(1) << 31)) return fail("rb_item_split_h: n too large");
  return launch_item_split_h(x, n, d, image, exps, group_max,
                             reinterpret_cast<hipStream_t>(stream));
}

namespace {
int check_items_h(const void* seq_img, const int* seq_exp, const void* item_img,
                  const int* item_exp, int64_t B, int64_t V, int64_t d) {
  if (!seq_exp || !item_exp) return fail("item scores (f16): null exponent pointer");
  return check_items("item scores (f16)", reinterpret_cast<const float*>(seq_img),
                     reinterpret_cast<const float*>(item_img), B, V, d);
}

// the rows variants' normaliser: 1 / (live rows of the whole call)
int check_inv_n(const char* fn, float inv_n) {
  if (!(inv_n > 0.0f) || !(inv_n <= 1.0f)) return fail(fn, "inv_n must be in (0, 1]");
  return 0;
}

// rows: rb_item_ce_fwd_h_rows, which also checks its inv_n and accumulate
int item_ce_fwd_h(const char* fn, bool rows, const void* seq_img, const int* seq_exp,
                  const void* item_img, const int* item_exp, const int64_t* target, int64_t B,
                  int64_t V, int64_t d, float inv_n, int accumulate, float* lse, float* loss,
                  void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = check_items_h(seq_img, seq_exp, item_img, item_exp, B, V, d)) return rc;
  if (!target || !lse || !loss || !workspace) return fail(fn, "null pointer");
  if (rows) {
    if (int rc = check_inv_n(fn, inv_n)) return rc;
    if (accumulate != 0 && accumulate != 1) return fail(fn, "accumulate must be 0 or 1");
  }
  return launch_item_ce_fwd_h(seq_img, seq_exp, item_img, item_exp, target, B, V, d, lse, loss,
                              workspace, workspace_bytes, rows, inv_n, accumulate,
                              as_stream(stream));
}

// The five rb_item_ce_probs_h* entry points.  want_p / want_pt: the layouts
// entry point fn writes; each needs its buffer, P^T its item group maxima and
// both together the row group maxima too.
int item_ce_probs_h(const char* fn, bool want_p, bool want_pt, const void* seq_img,
                    const int* seq_exp, const void* item_img, const int* item_exp,
                    const int64_t* target, const float* lse, const float* dloss, int64_t B,
                    int64_t V, int64_t d, int64_t item_offset, const CeProbsOut& o, void* stream) {
  if (int rc = check_items_h(seq_img, seq_exp, item_img, item_exp, B, V, d)) return rc;
  if (!target || !lse || !dloss || (want_p && !o.p) || (want_pt && (!o.pt || !o.item_max)) ||
      (want_p && want_pt && !o.row_max))
    return fail(fn, "null pointer");
  if (o.rows)
    if (int rc = check_inv_n(fn, o.inv_n)) return rc;
  if (want_p && o.ld < V) return fail(fn, "ld < V");
  if (want_pt && (o.ldt < B || o.ldt % 4 || reinterpret_cast<uintptr_t>(o.pt) % 16))
    return fail(fn, "probs_t must be 16-B aligned with ldt >= B, ldt % 4 == 0");
  return launch_item_ce_probs_h(seq_img, seq_exp, item_img, item_exp, target, lse, dloss, B, V, d,
                                item_offset, o, as_stream(stream));
}
}  // namespace

int rb_item_ce_fwd_h(const void* seq_img, const int* seq_exp, const void* item_img,
                     const int* item_exp, const int64_t* target, int64_t B, int64_t V, int64_t d,
                     float* lse, float* loss, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  return item_ce_fwd_h("rb_item_ce_fwd_h", false, seq_img, seq_exp, item_img, item_exp, target, B,
                       V, d, 0.0f, 0, lse, loss, workspace, workspace_bytes, stream);
}

int rb_item_ce_probs_h(const void* seq_img, const int* seq_exp, const void* item_img,
                       const int* item_exp, const int64_t* target, const float* lse,
                       const float* dloss, int64_t B, int64_t V, int64_t d, int64_t item_offset,
                       float* probs, int64_t ld, void* stream) {
  return item_ce_probs_h("rb_item_ce_probs_h", true, false, seq_img, seq_exp, item_img, item_exp,
                         target, lse, dloss, B, V, d, item_offset, {.p = probs, .ld = ld}, stream);
}

int rb_item_ce_probs_h_t(const void* seq_img, const int* seq_exp, const void* item_img,
                         const int* item_exp, const int64_t* target, const float* lse,
                         const float* dloss, int64_t B, int64_t V, int64_t d, int64_t item_offset,
                         float* probs_t, int64_t ldt, float* group_max, void* stream) {
  return item_ce_probs_h("rb_item_ce_probs_h_t", false, true, seq_img, seq_exp, item_img,
                         item_exp, target, lse, dloss, B, V, d, item_offset,
                         {.pt = probs_t, .ldt = ldt, .item_max = group_max}, stream);
}

int rb_item_ce_probs_h_both(const void* seq_img, const int* seq_exp, const void* item_img,
                            const int* item_exp, const int64_t* target, const float* lse,
                            const float* dloss, int64_t B, int64_t V, int64_t d,
                            int64_t item_offset, float* probs, int64_t ld, float* probs_t,
                            int64_t ldt, float* row_group_max, float* item_group_max,
                            void* stream) {
  return item_ce_probs_h("rb_item_ce_probs_h_both", true, true, seq_img, seq_exp, item_img,
                         item_exp, target, lse, dloss, B, V, d, item_offset,
                         {.p = probs, .ld = ld, .pt = probs_t, .ldt = ldt,
                          .row_max = row_group_max, .item_max = item_group_max},
                         stream);
}

// ---- include/recblr_dense.h: the all-position training loss -------------------------
int rb_item_ce_fwd_h_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                          const int* item_exp, const int64_t* target, int64_t B, int64_t V,
                          int64_t d, float inv_n, int accumulate, float* lse, float* loss,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  return item_ce_fwd_h("rb_item_ce_fwd_h_rows", true, seq_img, seq_exp, item_img, item_exp,
                       target, B, V, d, inv_n, accumulate, lse, loss, workspace, workspace_bytes,
                       stream);
}

int rb_item_ce_probs_h_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                            const int* item_exp, const int64_t* target, const float* lse,
                            const float* dloss, float inv_n, int64_t B, int64_t V, int64_t d,
                            int64_t item_offset, float* probs, int64_t ld, void* stream) {
  return item_ce_probs_h("rb_item_ce_probs_h_rows", true, false, seq_img, seq_exp, item_img,
                         item_exp, target, lse, dloss, B, V, d, item_offset,
                         {.p = probs, .ld = ld, .rows = true, .inv_n = inv_n}, stream);
}

int rb_item_ce_probs_h_both_rows(const void* seq_img, const int* seq_exp, const void* item_img,
                                 const int* item_exp, const int64_t* target, const float* lse,
                                 const float* dloss, float inv_n, int64_t B, int64_t V, int64_t d,
                                 int64_t item_offset, float* probs, int64_t ld, float* probs_t,
                                 int64_t ldt, float* row_group_max, float* item_group_max,
                                 void* stream) {
  return item_ce_probs_h("rb_item_ce_probs_h_both_rows", true, true, seq_img, seq_exp, item_img,
                         item_exp, target, lse, dloss, B, V, d, item_offset,
                         {.p = probs, .ld = ld, .pt = probs_t, .ldt = ldt,
                          .row_max = row_group_max, .item_max = item_group_max, .rows = true,
                          .inv_n = inv_n},
                         stream);
}

int rb_next_item_targets(const int64_t* ids, const int64_t* seq_offsets, const int64_t* order,
                         const int64_t* pos_items, int64_t B, int64_t ntok, int64_t m_pad,
                         int64_t* targets, void* stream) {
  if (!ids || !seq_offsets || !order || !pos_items || !targets)
    return fail("rb_next_item_targets: null pointer");
  if (B < 1 || ntok < 1 || m_pad < ntok) return fail("rb_next_item_targets: need B, ntok >= 1 and m_pad >= ntok");
  if ((m_pad + 255) / 256 > 0x7fffffffLL) return fail("rb_next_item_targets: grid too large");
  return launch_next_item_targets(ids, seq_offsets, order, pos_items, B, ntok, m_pad, targets,
                                  reinterpret_cast<hipStream_t>(stream));
}

// ---- the sampled pairwise loss (include/recblr_pairs.h) ---------------------------
namespace {
// both samplers; alias: the proposal's table, NULL for the uniform draw
int sample_negatives(const char* fn, const int64_t* item_seq, int64_t seq_rs,
                     const int64_t* lengths, const int64_t* pos_items, const int64_t* offsets,
                     const int64_t* inv, int64_t B, int64_t L, int64_t n_neg, int64_t first_item,
                     int64_t V, uint64_t seed, int64_t ntok, int64_t m_pad, const int64_t* alias,
                     int64_t* neg, void* stream) {
  if (!item_seq || !lengths || !pos_items || !neg) return fail(fn, "null pointer");
  if ((offsets == nullptr) != (inv == nullptr))
    return fail(fn, "offsets and inv must be given together");
  if (B < 1 || L < 1 || L > 8191 || seq_rs < L) return fail(fn, "need B >= 1, 1 <= L <= 8191, seq_rs >= L");
  if (n_neg < 1 || n_neg > 256) return fail(fn, "n_neg must be in [1, 256]");
  if (first_item < 0 || V <= first_item || V >= (int64_t(1) << 31))
    return fail(fn, "need 0 <= first_item < V < 2^31");
  if (offsets ? (ntok < 1 || m_pad < ntok || ntok > B * L) : (ntok != B || m_pad != B))
    return fail(fn, "need 1 <= ntok <= m_pad (packed rows), or ntok = m_pad = B (last position only)");
  if (B >= (int64_t(1) << 31) || B + ((m_pad - ntok) * n_neg + 255) / 256 > 0x7fffffffLL)
    return fail(fn, "grid too large");
  return launch_sample_negatives(item_seq, seq_rs, lengths, pos_items, offsets, inv, B, L, n_neg,
                                 first_item, V, seed, ntok, m_pad, alias, neg, as_stream(stream));
}
}  // namespace

int rb_sample_negatives(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                        const int64_t* pos_items, const int64_t* offsets, const int64_t* inv,
                        int64_t B, int64_t L, int64_t n_neg, int64_t first_item, int64_t V,
                        uint64_t seed, int64_t ntok, int64_t m_pad, int64_t* neg, void* stream) {
  return sample_negatives("rb_sample_negatives", item_seq, seq_rs, lengths, pos_items, offsets,
                          inv, B, L, n_neg, first_item, V, seed, ntok, m_pad, nullptr, neg, stream);
}

int rb_sample_negatives_alias(const int64_t* item_seq, int64_t seq_rs, const int64_t* lengths,
                              const int64_t* pos_items, const int64_t* offsets,
                              const int64_t* inv, int64_t B, int64_t L, int64_t n_neg,
                              int64_t first_item, int64_t V, uint64_t seed, int64_t ntok,
                              int64_t m_pad, const int64_t* alias, int64_t* neg, void* stream) {
  const char* fn = "rb_sample_negatives_alias";
  if (!alias) return fail(fn, "null pointer");
  if (reinterpret_cast<uintptr_t>(alias) % 8) return fail(fn, "alias must be 8-B aligned");
  return sample_negatives(fn, item_seq, seq_rs, lengths, pos_items, offsets, inv, B, L, n_neg,
                          first_item, V, seed, ntok, m_pad, alias, neg, stream);
}

int64_t rb_pair_loss_workspace(int64_t M) { return M <= 0 ? 0 : pair_loss_workspace_bytes(M); }

namespace {
int check_pairs(const char* fn, int64_t M, int64_t d, int64_t V, int64_t n_neg, float gamma) {
  if (M < 1 || V < 1) return fail(fn, "M and V must be positive");
  if (d < 4 || d > 512 || d % 4) return fail(fn, "d must be a multiple of 4 in [4, 512]");
  if (n_neg < 1 || n_neg > 16) return fail(fn, "n_neg must be in [1, 16]");
  if (!(gamma >= 0.0f)) return fail(fn, "gamma must be >= 0");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 31)) return fail(fn, "M or V too large");
  return 0;
}
}  // namespace

int rb_pair_loss_fwd(const float* h, int64_t ldh, const float* table, const int64_t* pos,
                     const int64_t* neg, int64_t M, int64_t d, int64_t V, int64_t n_neg,
                     float gamma, float* diff, float* loss, int64_t* n_live, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  const char* fn = "rb_pair_loss_fwd";
  if (!h || !table || !pos || !neg || !diff || !loss || !n_live || !workspace)
    return fail(fn, "null pointer");
  if (int rc = check_pairs(fn, M, d, V, n_neg, gamma)) return rc;
  if (ldh < d || ldh % 4 || !aligned16(h) || !aligned16(table))
    return fail(fn, "h and table must be 16-B aligned with ldh >= d, ldh % 4 == 0");
  if (workspace_bytes < pair_loss_workspace_bytes(M) || !aligned16(workspace))
    return fail(fn, "workspace too small or misaligned");
  return launch_pair_loss_fwd(h, ldh, table, pos, neg, M, d, V, n_neg, gamma, diff, loss, n_live,
                              workspace, as_stream(stream));
}

int rb_pair_loss_bwd(const float* table, const int64_t* pos, const int64_t* neg,
                     const float* diff, const float* dloss, const int64_t* n_live, int64_t M,
                     int64_t d, int64_t V, int64_t n_neg, float gamma, float* dh, float* coef,
                     void* stream) {
  const char* fn = "rb_pair_loss_bwd";
  if (!table || !pos || !neg || !diff || !dloss || !n_live || !dh || !coef)
    return fail(fn, "null pointer");
  if (int rc = check_pairs(fn, M, d, V, n_neg, gamma)) return rc;
  if (!aligned16(table) || !aligned16(dh)) return fail(fn, "table and dh must be 16-B aligned");
  return launch_pair_loss_bwd(table, pos, neg, diff, dloss, n_live, M, d, V, n_neg, gamma, dh,
                              coef, as_stream(stream));
}

int rb_embedding_bwd_apply_scaled(const float* src, int64_t src_ld, int64_t src_rows,
                                  const float* coef, int64_t M, int64_t d, int64_t V,
                                  int64_t padding_idx, float* dweight, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  const char* fn = "rb_embedding_bwd_apply_scaled";
  if (!src || !coef || !dweight || !workspace) return fail(fn, "null pointer");
  if (M <= 0 || d <= 0 || V <= 0) return fail(fn, "M, d, V must be positive");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 30)) return fail(fn, "M or V too large");
  if (src_rows < 1 || src_rows >= (int64_t(1) << 31) || src_ld < d)
    return fail(fn, "need 1 <= src_rows < 2^31 and src_ld >= d");
  return launch_embedding_apply_scaled(src, src_ld, src_rows, coef, M, d, V, padding_idx, dweight,
                                       workspace, workspace_bytes, as_stream(stream));
}

// ---- sampled softmax, negatives shared per sequence (include/recblr_pairs.h) --------
namespace {
int check_shared(const char* fn, int64_t M, int64_t B, int64_t d, int64_t V, int64_t n_neg,
                 int64_t max_len, float shift) {
  if (M < 1 || B < 1 || V < 1 || max_len < 1) return fail(fn, "M, B, V and max_len must be positive");
  if (d < 16 || d > 224 || d % 16) return fail(fn, "d must be a multiple of 16 in [16, 224]");
  if (n_neg < 1 || n_neg > 256) return fail(fn, "n_neg must be in [1, 256]");
  if (!(shift - shift == 0.0f)) return fail(fn, "shift must be finite");
  if (M >= (int64_t(1) << 31) || V >= (int64_t(1) << 31) || B >= (int64_t(1) << 22))
    return fail(fn, "M, V or B too large");
  return 0;
}

// the forward and the backward, with (items) and without the per-item
// correction: item_shift is then required, else it is NULL
int shared_softmax_fwd(const char* fn, bool items, const float* h, int64_t ldh,
                       const float* table, const int64_t* target, const int64_t* neg,
                       const int64_t* offsets, const int64_t* order, int64_t M, int64_t B,
                       int64_t d, int64_t V, int64_t n_neg, int64_t max_len, float shift,
                       const float* item_shift, float* lse, float* z0, float* loss,
                       int64_t* n_live, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!h || !table || !target || !neg || !offsets || !order || !lse || !z0 || !loss || !n_live ||
      !workspace || (items && !item_shift))
    return fail(fn, "null pointer");
  if (int rc = check_shared(fn, M, B, d, V, n_neg, max_len, shift)) return rc;
  if (ldh < d || ldh % 4 || !aligned16(h) || !aligned16(table))
    return fail(fn, "h and table must be 16-B aligned with ldh >= d, ldh % 4 == 0");
  if (workspace_bytes < shared_softmax_workspace_bytes(B, max_len) || !aligned16(workspace))
    return fail(fn, "workspace too small or misaligned");
  return launch_shared_softmax_fwd(h, ldh, table, target, neg, offsets, order, M, B, d, V, n_neg,
                                   max_len, shift, item_shift, lse, z0, loss, n_live, workspace,
                                   as_stream(stream));
}

int shared_softmax_bwd(const char* fn, bool items, const float* h, int64_t ldh,
                       const float* table, const int64_t* target, const int64_t* neg,
                       const int64_t* offsets, const int64_t* order, const float* lse,
                       const float* dloss, const int64_t* n_live, int64_t M, int64_t B, int64_t d,
                       int64_t V, int64_t n_neg, int64_t max_len, float shift,
                       const float* item_shift, float* dh, float* coef, float* dneg,
                       void* stream) {
  if (!h || !table || !target || !neg || !offsets || !order || !lse || !dloss || !n_live || !dh ||
      !coef || !dneg || (items && !item_shift))
    return fail(fn, "null pointer");
  if (int rc = check_shared(fn, M, B, d, V, n_neg, max_len, shift)) return rc;
  if (ldh < d || ldh % 4 || !aligned16(h) || !aligned16(table))
    return fail(fn, "h and table must be 16-B aligned with ldh >= d, ldh % 4 == 0");
  return launch_shared_softmax_bwd(h, ldh, table, target, neg, offsets, order, lse, dloss, n_live,
                                   M, B, d, V, n_neg, max_len, shift, item_shift, dh, coef, dneg,
                                   as_stream(stream));
}
}  // namespace

int64_t rb_shared_softmax_workspace(int64_t B, int64_t max_len) {
  return B <= 0 || B >= (int64_t(1) << 22) ? 0 : shared_softmax_workspace_bytes(B, max_len);
}

int rb_shared_softmax_fwd(const float* h, int64_t ldh, const float* table,
                          const int64_t* target, const int64_t* neg, const int64_t* offsets,
                          const int64_t* order, int64_t M, int64_t B, int64_t d, int64_t V,
                          int64_t n_neg, int64_t max_len, float shift, float* lse, float* z0,
                          float* loss, int64_t* n_live, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  return shared_softmax_fwd("rb_shared_softmax_fwd", false, h, ldh, table, target, neg, offsets,
                            order, M, B, d, V, n_neg, max_len, shift, nullptr, lse, z0, loss,
                            n_live, workspace, workspace_bytes, stream);
}

int rb_shared_softmax_fwd_items(const float* h, int64_t ldh, const float* table,
                                const int64_t* target, const int64_t* neg,
                                const int64_t* offsets, const int64_t* order, int64_t M,
                                int64_t B, int64_t d, int64_t V, int64_t n_neg, int64_t max_len,
                                float shift, const float* item_shift, float* lse, float* z0,
                                float* loss, int64_t* n_live, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return shared_softmax_fwd("rb_shared_softmax_fwd_items", true, h, ldh, table, target, neg,
                            offsets, order, M, B, d, V, n_neg, max_len, shift, item_shift, lse, z0,
                            loss, n_live, workspace, workspace_bytes, stream);
}

int rb_shared_softmax_bwd(const float* h, int64_t ldh, const float* table,
                          const int64_t* target, const int64_t* neg, const int64_t* offsets,
                          const int64_t* order, const float* lse, const float* dloss,
                          const int64_t* n_live, int64_t M, int64_t B, int64_t d, int64_t V,
                          int64_t n_neg, int64_t max_len, float shift, float* dh, float* coef,
                          float* dneg, void* stream) {
  return shared_softmax_bwd("rb_shared_softmax_bwd", false, h, ldh, table, target, neg, offsets,
                            order, lse, dloss, n_live, M, B, d, V, n_neg, max_len, shift, nullptr,
                            dh, coef, dneg, stream);
}

int rb_shared_softmax_bwd_items(const float* h, int64_t ldh, const float* table,
                                const int64_t* target, const int64_t* neg,
                                const int64_t* offsets, const int64_t* order, const float* lse,
                                const float* dloss, const int64_t* n_live, int64_t M, int64_t B,
                                int64_t d, int64_t V, int64_t n_neg, int64_t max_len, float shift,
                                const float* item_shift, float* dh, float* coef, float* dneg,
                                void* stream) {
  return shared_softmax_bwd("rb_shared_softmax_bwd_items", true, h, ldh, table, target, neg,
                            offsets, order, lse, dloss, n_live, M, B, d, V, n_neg, max_len, shift,
                            item_shift, dh, coef, dneg, stream);
}

// ---- candidate-list scoring (include/recblr_candidates.h) ---------------------------
namespace {
// what the three share: h, table, cand and their sizes (B >= 1 here)
int check_candidates(const char* fn, const float* h, int64_t ldh, const float* table,
                     const int64_t* cand, int64_t C, int64_t d, int64_t V) {
  if (!h || !table || !cand) return fail(fn, "null pointer");
  if (C < 1) return fail(fn, "C must be positive");
  if (V < 1 || V >= (int64_t(1) << 31)) return fail(fn, "need 1 <= V < 2^31");
  if (d < 4 || d > 512 || d % 4) return fail(fn, "d must be a multiple of 4 in [4, 512]");
  if (ldh < d || ldh % 4 || !aligned16(h) || !aligned16(table))
    return fail(fn, "h and table must be 16-B aligned with ldh >= d, ldh % 4 == 0");
  return 0;
}
}  // namespace

int rb_candidate_scores(const float* h, int64_t ldh, const float* table, const int64_t* cand,
                        int64_t B, int64_t C, int64_t d, int64_t V, float* scores,
                        void* stream) {
  const char* fn = "rb_candidate_scores";
  if (B < 0) return fail(fn, "B must be >= 0");
  if (B == 0) return 0;
  if (int rc = check_candidates(fn, h, ldh, table, cand, C, d, V)) return rc;
  if (!scores) return fail(fn, "null pointer");
  if (B >= (int64_t(1) << 31) || C >= (int64_t(1) << 31) || B * C >= (int64_t(1) << 37))
    return fail(fn, "B * C must stay below 2^37");
  return launch_candidate_scores(h, ldh, table, cand, B, C, d, V, scores, as_stream(stream));
}

int rb_candidate_topk(const float* h, int64_t ldh, const float* table, const int64_t* cand,
                      int64_t B, int64_t C, int64_t d, int64_t V, int64_t first_item, int64_t k,
                      const int64_t* exclude, int64_t E, int64_t* ids, float* scores,
                      void* stream) {
  const char* fn = "rb_candidate_topk";
  if (B < 0) return fail(fn, "B must be >= 0");
  if (B == 0) return 0;
  if (int rc = check_candidates(fn, h, ldh, table, cand, C, d, V)) return rc;
  if (!ids || !scores) return fail(fn, "null pointer");
  if (C > 4096) return fail(fn, "C must be in [1, 4096]");
  if (E < 0 || E > 4096) return fail(fn, "E must be in [0, 4096]");
  if (E > 0 && !exclude) return fail(fn, "null pointer");
  if (k < 1 || k >= (int64_t(1) << 31)) return fail(fn, "k must be in [1, 2^31)");
  if (first_item < 0 || first_item > V) return fail(fn, "first_item must be in [0, V]");
  if (B >= (int64_t(1) << 31)) return fail(fn, "grid too large");
  return launch_candidate_topk(h, ldh, table, cand, B, C, d, V, first_item, k, exclude, E, ids,
                               scores, as_stream(stream));
}

int rb_candidate_ranks(const float* h, int64_t ldh, const float* table, const int64_t* target,
                       const int64_t* cand, int64_t B, int64_t C, int64_t d, int64_t V,
                       int64_t first_item, int64_t* n_greater, int64_t* n_equal, void* stream) {
  const char* fn = "rb_candidate_ranks";
  if (B < 0) return fail(fn, "B must be >= 0");
  if (B == 0) return 0;
  if (int rc = check_candidates(fn, h, ldh, table, cand, C, d, V)) return rc;
  if (!target || !n_greater || !n_equal) return fail(fn, "null pointer");
  if (first_item < 0 || first_item > V) return fail(fn, "first_item must be in [0, V]");
  if (B >= (int64_t(1) << 31) || C >= (int64_t(1) << 40) ||
      B * candidate_rank_chunks(C) >= (int64_t(1) << 31))
    return fail(fn, "grid too large");
  return launch_candidate_ranks(h, ldh, table, target, cand, B, C, d, V, first_item, n_greater,
                                n_equal, as_stream(stream));
}

int rb_group_absmax(const float* x, int64_t n, int64_t c, int64_t ld, float* out, void* stream) {
  if (!x || !out) return fail("rb_group_absmax: null pointer");
  if (n <= 0 || c <= 0 || ld < c) return fail("rb_group_absmax: bad shape");
  return launch_group_absmax(x, n, c, ld, out, reinterpret_cast<hipStream_t>(stream));
}

int rb_item_scores(const float* seq, const float* items, int64_t B, int64_t V, int64_t d,
                   float* scores, void* stream) {
  if (int rc = check_items("rb_item_scores", seq, items, B, V, d)) return rc;
  if (!scores) return fail("rb_item_scores: null pointer");
  return launch_item_scores(seq, items, B, V, d, scores, reinterpret_cast<hipStream_t>(stream));
}

int rb_pad_prefix_fwd(const float* conv_b, const float* gate_w, const float* gate_b,
                      const float* lam, const int64_t* pad, int64_t pad_len, int64_t n_rows,
                      int64_t H, float* h0, float* workspace, void* stream) {
  if (!conv_b || !gate_w || !gate_b || !lam || !h0 || !workspace)
    return fail("rb_pad_prefix_fwd: null pointer");
  if (H <= 0 || H > 4096 || n_rows <= 0 || pad_len < 0)
    return fail("rb_pad_prefix_fwd: need 0 < H <= 4096, n_rows > 0, pad_len >= 0");
  return launch_pad_prefix_fwd(conv_b, gate_w, gate_b, lam, pad, pad_len, n_rows, H, h0,
                               workspace, reinterpret_cast<hipStream_t>(stream));
}

int rb_pad_prefix_bwd(const float* conv_b, const float* gate_w, const float* gate_b,
                      const float* lam, const int64_t* pad, int64_t pad_len, int64_t n_rows,
                      int64_t H, const float* dh0, float* dconv_b, float* dgate_w,
                      float* dgate_b, float* dlam, float* workspace, int accumulate,
                      void* stream) {
  if (!conv_b || !gate_w || !gate_b || !lam || !dh0 || !dconv_b || !dgate_w || !dgate_b || !dlam ||
      !workspace)
    return fail("rb_pad_prefix_bwd: null pointer");
  if (H <= 0 || H > 4096 || n_rows <= 0 || pad_len < 0)
    return fail("rb_pad_prefix_bwd: need 0 < H <= 4096, n_rows > 0, pad_len >= 0");
  return launch_pad_prefix_bwd(conv_b, gate_w, gate_b, lam, pad, pad_len, n_rows, H, dh0,
                               dconv_b, dgate_w, dgate_b, dlam, workspace, accumulate,
                               reinterpret_cast<hipStream_t>(stream));
}

int rb_colsum(const float* in, int64_t M, int64_t P, int64_t C, int64_t rs, int64_t ms,
              float* out, void* stream) {
  if (!in || !out) return fail("rb_colsum: null pointer");
  if (M <= 0 || P <= 0 || C <= 0 || rs < C || (M > 1 && ms < P * rs))
    return fail("rb_colsum: bad shape or strides");
  if (M * ((C + 63) / 64) > 0x7fffffffLL) return fail("rb_colsum: grid too large");
  return launch_colsum(in, M, P, C, rs, ms, out, reinterpret_cast<hipStream_t>(stream));
}

int rb_colsum_chunked(const float* in, int64_t M, int64_t P, int64_t C, int64_t rs,
                      int64_t chunk_rows, float* part, uint32_t* counters, int64_t n_counters,
                      float* out, void* stream) {
  if (!in || !out || !part || !counters) return fail("rb_colsum_chunked: null pointer");
  if (M <= 0 || P <= 0 || C <= 0 || rs < C ||
      (chunk_rows != 64 && chunk_rows != 128 && chunk_rows != 256) || P % chunk_rows)
    return fail("rb_colsum_chunked: bad shape, stride or chunk size");
  const int64_t cblocks = (C + 63) / 64;
  if (n_counters < M * cblocks) return fail("rb_colsum_chunked: too few counters");
  if (M * cblocks * (P / chunk_rows) > 0x7fffffffLL || M * P * rs >= ((int64_t)1 << 40))
    return fail("rb_colsum_chunked: grid too large");
  return launch_colsum_chunked(in, M, P, C, rs, (int)chunk_rows, part,
                               reinterpret_cast<unsigned*>(counters), out,
                               reinterpret_cast<hipStream_t>(stream));
}

int rb_pack_plan(const int64_t* item_seq, int64_t seq_rs, const int64_t* seq_offsets,
                 const int64_t* order, int64_t B, int64_t L, int64_t* ids, int64_t* row_pos,
                 int64_t* inv, int64_t* last, void* stream) {
  if (!item_seq || !seq_offsets || !order || !ids || !row_pos || !inv || !last)
    return fail("rb_pack_plan: null pointer");
  if (B < 1 || L < 1 || seq_rs < L) return fail("rb_pack_plan: bad shape or row stride");
  if ((B + 3) / 4 > 0x7fffffffLL) return fail("rb_pack_plan: grid too large");
  return launch_pack_plan(item_seq, seq_rs, seq_offsets, order, B, ids, row_pos, inv, last,
                          reinterpret_cast<hipStream_t>(stream));
}

int64_t rb_gemm_h_weight_bytes(int64_t C, int64_t R) {
  // + the weight-stationary kernel's planes where it can run (R % 32 == 0)
  return ws_image_offset(C, R) + (R % 32 == 0 ? C * R * 4 : 0);
}
int rb_gemm_nt_h_mode(int mode) { return gemm_nt_h_mode(mode); }

int rb_gemm_nt_h_ln(const float* A, int64_t lda, int64_t M, int64_t R, const void* Wf, int64_t C,
                    const float* bias, const float* resid, const float* gamma, const float* beta,
                    float eps, uint64_t seed, float p, float* y, float* s_out, float* mean,
                    float* rstd, int64_t ldo, float* rmax, void* stream) {
  if (!A || !Wf || !resid || !gamma || !beta || !y || !s_out || !mean || !rstd)
    return fail("rb_gemm_nt_h_ln: null pointer");
  if (M <= 0 || R <= 0 || C != 128) return fail("rb_gemm_nt_h_ln: C must be 128, M and R positive");
  if (R != 128 && R != 256 && R != 512) return fail("rb_gemm_nt_h_ln: R must be 128, 256 or 512");
  if (lda < R || lda % 4 || ldo < C || ldo % 4) return fail("rb_gemm_nt_h_ln: bad row strides");
  if (!aligned16(A) || !aligned16(Wf) || !aligned16(resid) || !aligned16(y) || !aligned16(s_out) ||
      !aligned16(gamma) || !aligned16(beta) || (bias && !aligned16(bias)))
    return fail("rb_gemm_nt_h_ln: A, Wf, resid, y, s_out, gamma, beta and bias must be 16-byte aligned");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_gemm_nt_h_ln: dropout p must be in [0, 1)");
  if (!(eps > 0.0f)) return fail("rb_gemm_nt_h_ln: eps must be positive");
  if ((M + 31) / 32 > 0x3fffffffLL) return fail("rb_gemm_nt_h_ln: grid too large");
  if (gemm_nt_h_mode(-1) != 1) return fail("rb_gemm_nt_h_ln: needs the weight-stationary kernel (rb_gemm_nt_h_mode 1)");
  return launch_gemm_nt_ws_ln(A, lda, M, (int)R, Wf, (int)C, bias, resid, make_drop(nullptr, seed, p),
                              gamma, beta, eps, y, s_out, mean, rstd, ldo, rmax,
                              reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_h_split_weights(const rb_split_job* jobs, int64_t n, void* stream) {
  if (!jobs || n < 1 || n > RB_MAX_SPLIT_JOBS)
    return fail("rb_gemm_h_split_weights: need 1..RB_MAX_SPLIT_JOBS jobs");
  for (int64_t j = 0; j < n; ++j) {
    const rb_split_job& b = jobs[j];
    if (!b.W || !b.Wf) return fail("rb_gemm_h_split_weights: null pointer");
    if (b.C <= 0 || b.R <= 0 || b.C % 32 || b.R % 16 || b.C > (1 << 20) || b.R > (1 << 20))
      return fail("rb_gemm_h_split_weights: C must be a multiple of 32 and R of 16");
    if (b.ldw < (b.transpose ? b.C : b.R)) return fail("rb_gemm_h_split_weights: bad row stride");
    if (!aligned16(b.Wf)) return fail("rb_gemm_h_split_weights: Wf must be 16-byte aligned");
  }
  return launch_split_weights_h(jobs, (int)n, reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_nt_h(const float* A, int64_t lda, int64_t M, int64_t R, const void* Wf, int64_t C,
                 const float* bias, float* out, int64_t ldo, int accumulate, float* rmax,
                 void* stream) {
  if (!A || !Wf || !out) return fail("rb_gemm_nt_h: null pointer");
  if (M <= 0 || R <= 0 || C <= 0) return fail("rb_gemm_nt_h: empty shape");
  if (accumulate) return fail("rb_gemm_nt_h: accumulate is not supported (add the residual in its consumer)");
  if (R % 32 || C % 32 || R > (1 << 16) || C > 1024)
    return fail("rb_gemm_nt_h: R and C must be multiples of 32 (C <= 1024)");
  if (lda < R || lda % 4 || ldo < C || ldo % 2) return fail("rb_gemm_nt_h: bad row strides");
  if (!aligned16(A) || !aligned16(Wf) || (reinterpret_cast<uintptr_t>(out) & 7))
    return fail("rb_gemm_nt_h: A and Wf must be 16-byte aligned, out 8-byte aligned");
  if ((M + 31) / 32 > 0x7fffffffLL) return fail("rb_gemm_nt_h: grid too large");
  return launch_gemm_nt_h(A, lda, M, (int)R, Wf, (int)C, bias, out, ldo, accumulate, rmax,
                          reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_nt_h_act(const float* A, int64_t lda, int64_t M, int64_t R, const void* Wf, int64_t C,
                     const float* bias, float* out, int64_t ldo, float* rmax, float* act,
                     uint64_t seed, float p, void* stream) {
  if (!A || !Wf || !out || !act) return fail("rb_gemm_nt_h_act: null pointer");
  if (M <= 0 || R <= 0 || C <= 0) return fail("rb_gemm_nt_h_act: empty shape");
  if (R % 32 || C % 32 || R > 1024 || C > 1024)
    return fail("rb_gemm_nt_h_act: R and C must be multiples of 32 (R, C <= 1024)");
  if (lda < R || lda % 4 || ldo < C || ldo % 4) return fail("rb_gemm_nt_h_act: bad row strides");
  if (!aligned16(A) || !aligned16(Wf) || !aligned16(out) || !aligned16(act) ||
      (bias && !aligned16(bias)))
    return fail("rb_gemm_nt_h_act: A, Wf, out, act and bias must be 16-byte aligned");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_gemm_nt_h_act: dropout p must be in [0, 1)");
  if ((M + 31) / 32 > 0x7fffffffLL) return fail("rb_gemm_nt_h_act: grid too large");
  return launch_gemm_nt_h_act(A, lda, M, (int)R, Wf, (int)C, bias, out, ldo, rmax, act,
                              make_drop(nullptr, seed, p), reinterpret_cast<hipStream_t>(stream));
}

int rb_adam_step(const rb_adam_job* jobs, int64_t n, double lr, double beta1, double beta2,
                 double eps, double weight_decay, double bc1, double bc2, void* stream) {
  if (!jobs || n <= 0 || n > RB_MAX_ADAM_JOBS) return fail("rb_adam_step: 1..RB_MAX_ADAM_JOBS jobs");
  int64_t blocks = 0;
  for (int64_t j = 0; j < n; ++j) {
    const rb_adam_job& b = jobs[j];
    if (!b.param || !b.grad || !b.exp_avg || !b.exp_avg_sq || b.n <= 0)
      return fail("rb_adam_step: null pointer or empty tensor");
    if (!aligned16(b.param) || !aligned16(b.grad) || !aligned16(b.exp_avg) ||
        !aligned16(b.exp_avg_sq))
      return fail("rb_adam_step: tensors must be 16-byte aligned");
    blocks += (b.n + 1023) / 1024;
  }
  if (blocks > 0x7fffffffLL) return fail("rb_adam_step: too many elements");
  if (!(bc1 > 0.0 && bc2 > 0.0)) return fail("rb_adam_step: bias corrections must be > 0");
  return launch_adam(jobs, (int)n, lr, beta1, beta2, eps, weight_decay, bc1, bc2,
                     reinterpret_cast<hipStream_t>(stream));
}

int64_t rb_gemm_nt_h_dact_parts(void) { return nt_h_dact_parts(); }

int rb_gemm_nt_h_dact(const float* A, int64_t lda, int64_t M, int64_t R, const void* Wf, int64_t C,
                      float* out, int64_t ldo, float* rmax, const float* pre, uint64_t seed,
                      float p, float* dpart, int64_t n_parts, void* stream) {
  if (!A || !Wf || !out || !pre || !dpart) return fail("rb_gemm_nt_h_dact: null pointer");
  if (M <= 0 || R <= 0 || C <= 0) return fail("rb_gemm_nt_h_dact: empty shape");
  if (R % 32 || C % 32 || R > 1024 || C > 512)
    return fail("rb_gemm_nt_h_dact: R and C must be multiples of 32 (R <= 1024, C <= 512)");
  if (lda < R || lda % 4 || ldo < C || ldo % 4) return fail("rb_gemm_nt_h_dact: bad row strides");
  if (!aligned16(A) || !aligned16(Wf) || !aligned16(out) || !aligned16(pre) || !aligned16(dpart))
    return fail("rb_gemm_nt_h_dact: A, Wf, out, pre and dpart must be 16-byte aligned");
  if (!(p >= 0.0f && p < 1.0f)) return fail("rb_gemm_nt_h_dact: dropout p must be in [0, 1)");
  if ((M + 31) / 32 > 0x7fffffffLL) return fail("rb_gemm_nt_h_dact: grid too large");
  return launch_gemm_nt_h_dact(A, lda, M, (int)R, Wf, (int)C, out, ldo, rmax, pre,
                               make_drop(nullptr, seed, p), dpart, n_parts,
                               reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_tn_h(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t M, int64_t N,
                 int64_t K, const float* ymax, const float* xmax, float* parts, int64_t splits,
                 void* stream) {
  if (!dY || !X || !ymax || !xmax || !parts) return fail("rb_gemm_tn_h: null pointer");
  if (M <= 0 || N <= 0 || K <= 0) return fail("rb_gemm_tn_h: empty shape");
  if (N % 128 || K % 128 || N > 65536 || K > 65536)
    return fail("rb_gemm_tn_h: N and K must be multiples of 128 (<= 65536)");
  if (splits < 1 || splits > 65536) return fail("rb_gemm_tn_h: splits must be in [1, 65536]");
  if (ldy < N || ldx < K || ldy % 4 || ldx % 4) return fail("rb_gemm_tn_h: bad row strides");
  if (!aligned16(dY) || !aligned16(X)) return fail("rb_gemm_tn_h: dY and X must be 16-byte aligned");
  if ((N / 128) * (K / 128) * splits > 0x7fffffffLL) return fail("rb_gemm_tn_h: grid too large");
  // the kernel reads a row chunk through a buffer descriptor: 32-bit record
  // count and lane offsets over the chunk's bytes (launch_gemm_tn_h's chunk)
  const int64_t mk = ((M + splits - 1) / splits + 31) / 32 * 32;
  if (mk * (ldy > ldx ? ldy : ldx) * 4 >= 0x7fffffffLL)
    return fail("rb_gemm_tn_h: a row chunk spans 2 GiB or more (use more splits)");
  return launch_gemm_tn_h(dY, ldy, X, ldx, M, (int)N, (int)K, ymax, xmax, parts, (int)splits,
                          reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_bf16_weight_image(const float* W, int64_t ldw, int64_t C, int64_t R, int transpose,
                              void* img, void* stream) {
  if (!W || !img) return fail("rb_gemm_bf16_weight_image: null pointer");
  if (C <= 0 || R <= 0 || C % 16 || R % 32 || C > 65536 || R > 65536)
    return fail("rb_gemm_bf16_weight_image: C % 16 == 0 and R % 32 == 0 required (<= 65536)");
  if (ldw < (transpose ? C : R)) return fail("rb_gemm_bf16_weight_image: bad row stride");
  if (!aligned16(img)) return fail("rb_gemm_bf16_weight_image: img must be 16-byte aligned");
  return launch_bf16_weight_image(W, ldw, (int)C, (int)R, transpose ? 1 : 0, img,
                                  reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_nt_bf16(const void* A, int64_t lda, int64_t M, int64_t R, const void* img, int64_t C,
                    const float* bias, void* out, int64_t ldo, void* stream) {
  if (!A || !img || !out) return fail("rb_gemm_nt_bf16: null pointer");
  if (M <= 0 || R <= 0 || C <= 0) return fail("rb_gemm_nt_bf16: empty shape");
  if (R % 64 || C % 256 || R > 16384 || C > 65536)
    return fail("rb_gemm_nt_bf16: R % 64 == 0 (<= 16384) and C % 256 == 0 required");
  if (lda < R || lda % 8 || lda > (1 << 20) || ldo < C || ldo % 8)
    return fail("rb_gemm_nt_bf16: bad row strides (lda % 8 == 0, ldo % 8 == 0)");
  if (!aligned16(A) || !aligned16(img) || !aligned16(out) || (bias && !aligned16(bias)))
    return fail("rb_gemm_nt_bf16: A, img, out and bias must be 16-byte aligned");
  if ((M + 255) / 256 > 0x7fffffffLL / (C / 256) / 2) return fail("rb_gemm_nt_bf16: too many tiles");
  return launch_gemm_nt_bf16(A, lda, M, (int)R, img, (int)C, bias, out, ldo,
                             reinterpret_cast<hipStream_t>(stream));
}

int rb_gemm_tn_hs(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t M, int64_t N,
                  int64_t K, float* dw, int accumulate, void* stream) {
  if (!dY || !X || !dw) return fail("rb_gemm_tn_hs: null pointer");
  if (M <= 0 || N <= 0 || K <= 0) return fail("rb_gemm_tn_hs: empty shape");
  if (N % 32 || K % 32 || N > 65536 || K > 65536)
    return fail("rb_gemm_tn_hs: N and K must be multiples of 32");
  if (M > (1 << 24)) return fail("rb_gemm_tn_hs: M too large for the few-rows kernel");
  if (ldy < N || ldx < K) return fail("rb_gemm_tn_hs: bad row strides");
  return launch_gemm_tn_hs(dY, ldy, X, ldx, M, (int)N, (int)K, dw, accumulate,
                           reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"

// session_append_args.cpp — rb_session_append's and rb_session_step's argument
// checks under the host sanitizers, on a machine without a GPU: every call
// below fails a check, so it returns RB_EINVAL with its message before any
// HIP call, and no pointer is dereferenced (the layer array is the only real
// memory).  The checks the two entries share are exercised through both, each
// with its own message prefix.
//
// Build and run from the repository root (gfx950 code objects are compiled
// but never loaded):
//   hipcc -std=c++20 -O1 -g --offload-arch=gfx950 -ffp-contract=off -I include \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -o tools/bin/session_append_args tools/session_append_args.cpp \
//     datamining_recblr_amd/session/*.hip
//   tools/bin/session_append_args
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../datamining_recblr_amd/session/recblr_session.h"

namespace {

struct Call {
  std::vector<rb_session_layer> layers;
  int64_t n_layers = 2;
  float* p = reinterpret_cast<float*>(256);   // non-null, 16-byte aligned, never dereferenced
  const float *emb = p, *ln_w = p, *ln_b = p;
  const int64_t* items = reinterpret_cast<const int64_t*>(256);
  int64_t* count = reinterpret_cast<int64_t*>(256);
  float *out = p, *y = p, *y_all = p;
  float eps = 1e-12f;
  int64_t B = 3, T = 4, N = 8, V = 50, d = 64, H = 128, K = 4;
  bool null_layers = false;
  bool step = false;   // through rb_session_step (no y_all, no T)

  Call() : layers(2) {
    for (rb_session_layer& L : layers) {
      float* f = p;
      L = rb_session_layer{f, f, f, f, f, f, f, f, f, f, f, f, f, f, f, f, f, f};
    }
  }
  int run() const {
    if (step)
      return rb_session_step(null_layers ? nullptr : layers.data(), n_layers, emb, ln_w, ln_b, eps,
                             items, nullptr, count, out, y, nullptr, B, N, V, d, H, K, 0, 0,
                             nullptr);
    return rb_session_append(null_layers ? nullptr : layers.data(), n_layers, emb, ln_w, ln_b,
                             eps, items, nullptr, count, out, y, y_all, nullptr, B, T, N, V, d, H,
                             K, 0, 0, nullptr);
  }
};

int failures = 0;

void expect_one(const char* what, const Call& c, const std::string& message) {
  const int rc = c.run();
  const char* got = rb_session_last_error_string();
  if (rc != -1 || message != got) {
    std::printf("FAIL %s: rc %d, \"%s\" (want -1, \"%s\")\n", what, rc, got, message.c_str());
    ++failures;
  }
}

// `reason` is refused by rb_session_append and, with shared (a check of
// check_encoder_args), by rb_session_step too
void expect(const char* what, Call c, const char* reason, bool shared = true) {
  expect_one(what, c, std::string("rb_session_append: ") + reason);
  if (!shared) return;
  c.step = true;
  expect_one(what, c, std::string("rb_session_step: ") + reason);
}

}  // namespace

int main() {
  const char* kNull = "null pointer";
  const char* kShape = "d and H must be positive multiples of 16";
  Call c;
  c.null_layers = true; expect("layers", c, kNull);
  c = Call(); c.emb = nullptr; expect("emb", c, kNull);
  c = Call(); c.ln_w = nullptr; expect("ln_w", c, kNull);
  c = Call(); c.ln_b = nullptr; expect("ln_b", c, kNull);
  c = Call(); c.items = nullptr; expect("items", c, kNull);
  c = Call(); c.count = nullptr; expect("count", c, kNull);
  c = Call(); c.out = nullptr; expect("out", c, kNull);
  for (int64_t T : {0, 3, 5, 32, -16}) {
    c = Call(); c.T = T; expect("T", c, "T must be 1, 2, 4, 8 or 16", false);
  }
  for (int64_t K : {0, 9}) {
    c = Call(); c.K = K; expect("K", c, "conv kernel size K must be in [1, 8]");
  }
  c = Call(); c.d = 24; expect("d", c, kShape);
  c = Call(); c.H = 100; expect("H", c, kShape);
  for (int64_t n : {0, 9}) {
    c = Call(); c.n_layers = n; expect("n_layers", c, "n_layers must be in [1, 8]");
  }
  c = Call(); c.B = 0; expect("B", c, "B, N and V must be positive");
  c = Call(); c.B = int64_t(1) << 31; expect("B", c, "B, N and V must be < 2^31");
  c = Call(); c.d = 1024; c.H = 2048;
  expect("lds", c, "shape needs more LDS than a compute unit has (160 KiB)");
  c = Call(); c.eps = 0.0f; expect("eps", c, "eps must be positive");
  c = Call(); c.y = reinterpret_cast<float*>(264);
  expect("y", c, "emb, out and y must be 16-byte aligned");
  c = Call(); c.y_all = reinterpret_cast<float*>(264);
  expect("y_all", c, "y_all must be 16-byte aligned", false);
  // per layer: the second layer is reached
  c = Call(); c.layers[1].w_gate = nullptr; expect("w_gate", c, "null pointer in a layer");
  c = Call(); c.layers[1].conv_state = nullptr;
  expect("conv_state", c, "null conv pointer in a layer");
  c = Call(); c.layers[1].w2 = nullptr; expect("w2", c, "null ffn pointer in a layer");
  c = Call(); c.layers[1].w_in = reinterpret_cast<const float*>(264);
  expect("w_in", c, "weight matrices must be 16-byte aligned");
  if (failures)
    std::printf("%d check(s) failed\n", failures);
  else
    std::printf("rb_session_append, rb_session_step: every argument check refused as expected\n");
  return failures ? 1 : 0;
}

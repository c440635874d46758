// nt_plan.h — which launch takes which rows of an f16x3 NT GEMM call on the
// persistent kernel (gemm_half.hip: rb_gemm_nt_h, _act, _dact).  Plain C++,
// no HIP: the compute-unit count is an argument, so tools/nt_plan_check.cpp
// prints the plan on any machine (tests/test_nt_plan.py).
#pragma once

#include <algorithm>
#include <cstdint>

namespace rb {

constexpr int NT_WAVES = 8;           // waves per workgroup
constexpr int NT_BM = 32 * NT_WAVES;  // rows per tile
constexpr int NT_MAXC = 1024;         // columns whose exponents and bias fit the LDS
constexpr int NT_DACT_MAXC = 512;     // DACT's LDS column sums: 8 waves x C floats

// The persistent grid: one workgroup per CU, a multiple of 8 (the XCD pairing).
inline int nt_grid_max(int ncus) { return ncus / 8 * 8 * (8 / NT_WAVES); }

// Shapes the few-rows kernel (gemm_small.hip) measured faster on than one
// partial round of 256 x 64 tiles: a few thousand rows with K = 512, or
// C = 128 (tools/gemmbench_h.hip, profiles/r03_gemmbench_small_m.log) — at
// 8,192 rows it is 2.7x slower.
inline bool nt_few_rows(int64_t M, int R, int C) { return M <= 4096 && (R > 256 || C < 256); }

// The fused epilogues (ACT, DACT) take only the shapes whose every row runs
// on a wide-epilogue launch.  wide: out and the second operand (act / pre)
// 16-byte aligned, ldo % 4 == 0.
inline bool nt_h_act_ok(int64_t M, int R, int C, bool wide) {
  return wide && C % 256 == 0 && C <= NT_MAXC && R <= 1024 && !nt_few_rows(M, R, C);
}

enum class NtKind { plain, act, dact };

enum class NtPath {
  main,      // every row on the main tiles
  tail,      // every row on 256 x 64 tiles
  both,      // main tiles, then 256 x 64 tiles, in one launch (k_gemm_nt_h2)
  few,       // every row on the few-rows kernel
  few_main,  // the few-rows kernel for the rows past M_main, then the main launch
  error,
};

struct NtPlan {
  NtPath path;
  const char* err;        // path == error: the message
  int64_t M_main;         // rows [0, M_main) on the main tiles, [M_main, M) past them
  int nb;                 // the main tile's 32-column blocks: 4 (256 x 128) or 8 (256 x 256)
  bool wide, bias;        // the main kernel's WIDE and every kernel's BIAS
  int m_tiles, grid;      // the main launch (or phase)
  int m_tiles_t, grid_t;  // the 256 x 64 launch (or phase)
  // dact: the phases' first dpart rows are 0 and dpart_tail; rows from `used`
  // on are written by no workgroup
  int64_t dpart_tail, used;
};

// The persistent grid runs whole rounds of G0 tiles; the rows past the last
// whole round would run on a fraction of the chip (800 row tiles on 256 CUs:
// a fourth round on 32 of them, +18% time for +4% rows), so they run on
// 256 x 64 tiles (2-4x as many, each a fraction of the time), in the same
// launch where the output is wide.  Below one round, or for C % 128 != 0,
// every row goes to those tiles, or to the few-rows kernel where it wins
// (nt_few_rows), for C % 64 != 0 and for an output that is not wide.  When
// the column tiles do not divide G0, and for R > 1024 (beyond the few-rows
// kernel), the main launch takes every row, a partial round included.
// The three entries differ in the main tile (plain: 256 x 256 for a wide
// output with C % 256 == 0, else 256 x 128; act: 256 x 256; dact: 256 x 128)
// and in what they refuse; n_parts is dact's count of dpart rows.
inline NtPlan nt_plan(NtKind kind, int64_t M, int R, int C, bool wide, bool has_bias, int ncus,
                      int64_t n_parts = 0) {
  NtPlan p{};
  const auto error = [&p](const char* msg) {
    p.path = NtPath::error;
    p.err = msg;
    return p;
  };
  if (kind == NtKind::act && !nt_h_act_ok(M, R, C, wide))
    return error("rb_gemm_nt_h_act: shape or alignment without a wide-epilogue launch");
  if (kind == NtKind::dact && (!nt_h_act_ok(M, R, C, wide) || C > NT_DACT_MAXC))
    return error("rb_gemm_nt_h_dact: shape or alignment without a wide-epilogue launch");
  p.nb = kind == NtKind::act ? 8 : kind == NtKind::dact ? 4 : (wide && C % 256 == 0 ? 8 : 4);
  p.wide = wide;
  p.bias = has_bias && kind != NtKind::dact;
  const int G0 = nt_grid_max(ncus);
  const int nct0 = C % 128 ? 0 : C / (32 * p.nb);   // the main launch's column tiles
  if (R > 1024 && nct0 == 0) return error("rb_gemm_nt_h: C % 128 != 0 needs R <= 1024");
  const int64_t rows_round = nct0 ? (int64_t)(G0 / nct0) * NT_BM : 0;
  p.M_main = R > 1024 ? M
           : (nct0 && G0 % nct0 == 0 && rows_round > 0) ? M / rows_round * rows_round
                                                        : (nct0 ? M : 0);
  const bool few = p.M_main == 0 && nt_few_rows(M, R, C);
  const bool tiles = !few && wide && C % 64 == 0;   // the rows past M_main on 256 x 64 tiles
  p.path = p.M_main == M ? NtPath::main
         : tiles ? (p.M_main > 0 ? NtPath::both : NtPath::tail)
                 : (p.M_main > 0 ? NtPath::few_main : NtPath::few);
  const auto size = [&](int64_t rows, int cols, int& m_tiles, int& grid) {
    m_tiles = (int)((rows + NT_BM - 1) / NT_BM);
    const int64_t n_tiles = (int64_t)((m_tiles + 7) / 8) * 8 * (C / cols);
    grid = rows > 0 ? (int)std::min<int64_t>(n_tiles, (int64_t)G0) : 0;
  };
  size(p.M_main, 32 * p.nb, p.m_tiles, p.grid);
  if (tiles) size(M - p.M_main, 64, p.m_tiles_t, p.grid_t);
  if (kind == NtKind::dact) {
    p.dpart_tail = p.grid;
    p.used = (int64_t)p.grid + p.grid_t;
    if (p.used > n_parts) return error("rb_gemm_nt_h_dact: dpart has too few rows");
  }
  return p;
}

// dpart rows that hold every dact call (either phase at most one full grid)
inline int64_t nt_h_dact_parts(int ncus) { return 2 * (int64_t)nt_grid_max(ncus); }

}  // namespace rb

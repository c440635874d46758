// nt_plan_check — prints nt_plan() (csrc/nt_plan.h) as one line per case over
// a sweep of shapes and CU counts; tests/test_nt_plan.py compares the output
// with tests/golden/nt_plan_sweep.txt.gz.  Host C++ only:
//   c++ -std=c++17 -O1 -o nt_plan_check tools/nt_plan_check.cpp
#include <cstdio>

#include "../datamining_recblr_amd/csrc/nt_plan.h"

using namespace rb;

static const char* kKinds[] = {"plain", "act", "dact"};
static const char* kPaths[] = {"main", "tail", "both", "few", "few_main", "error"};

static void line(NtKind kind, int64_t M, int R, int C, int wide, int bias, int ncus,
                 int64_t n_parts) {
  const NtPlan p = nt_plan(kind, M, R, C, wide != 0, bias != 0, ncus, n_parts);
  std::printf("%s %lld %d %d %d %d %d %lld : ", kKinds[(int)kind], (long long)M, R, C, wide, bias,
              ncus, (long long)n_parts);
  if (p.path == NtPath::error)
    std::printf("error %s\n", p.err);
  else
    std::printf("%s %lld nb%d w%d b%d %d %d %d %d %lld %lld\n", kPaths[(int)p.path],
                (long long)p.M_main, p.nb, (int)p.wide, (int)p.bias, p.m_tiles, p.grid,
                p.m_tiles_t, p.grid_t, (long long)p.dpart_tail, (long long)p.used);
}

int main() {
  const int64_t Ms[] = {1, 31, 32, 33, 255, 256, 257, 2048, 4096, 4097, 8192, 16383, 16384,
                        16384 + 293, 32768 + 293, 65536, 65536 + 293, 70001, 196608 + 8024, 204632};
  const int Rs[] = {32, 128, 256, 288, 512, 1024, 1056};
  const int Cs[] = {32, 64, 96, 128, 256, 384, 512, 1024};
  const int cus[] = {256, 304, 64};   // 304, 64: G0 % (column tiles) goes both ways
  for (NtKind kind : {NtKind::plain, NtKind::act, NtKind::dact})
    for (int ncus : cus)
      for (int64_t M : Ms)
        for (int R : Rs)
          for (int C : Cs)
            for (int wide = 0; wide < 2; ++wide)
              for (int bias = 0; bias < 2; ++bias)
                line(kind, M, R, C, wide, bias, ncus,
                     kind == NtKind::dact ? nt_h_dact_parts(ncus) : 0);
  // dact's n_parts bound: one buffer row, one row short, exact, one to spare
  for (int ncus : cus)
    for (int64_t M : {(int64_t)5000, (int64_t)70001, (int64_t)196608, (int64_t)204632})
      for (int C : {256, 512}) {
        const int64_t used =
            nt_plan(NtKind::dact, M, 128, C, true, false, ncus, nt_h_dact_parts(ncus)).used;
        for (int64_t n_parts : {(int64_t)1, used - 1, used, used + 1})
          line(NtKind::dact, M, 128, C, 1, 0, ncus, n_parts);
      }
  return 0;
}

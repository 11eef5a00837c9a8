// Stand-alone check of the add + norm backward's host plan
// (videomamba_amd/csrc/vm_norm_bwd_plan.h): walks plan_norm_bwd() over a grid of shapes and
// exits non-zero unless the workgroups' row ranges cover [0, rows) exactly once in order with
// none empty, every (workgroup, which) region lies inside the reported size back to back, the
// reduce ranges cover the workgroups exactly once in order, and the size respects the
// documented bound.  Built and run by tests/test_train_bwd_cpu.py with
// -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>

#include "vm_norm_bwd_plan.h"

using namespace vm;

static long g_fail = 0;
static long long g_R;
static int g_C;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (g_fail++ < 20)                                                                     \
        std::fprintf(stderr, "line %d: %s  [rows=%lld cols=%d]\n", __LINE__, #cond, g_R, g_C); \
    }                                                                                        \
  } while (0)

int main() {
  const long long Rs[] = {0, 1, 3, 4, 5, 8, 257, 1569, 8191, 8192, 8193, 12552, 50208,
                          3000000, 5000000000LL};
  const int Cs[] = {0, 1, 3, 4, 63, 64, 65, 100, 192, 576, 1024, 2047, 2048};
  long plans = 0;
  for (long long R : Rs) for (int C : Cs) {
    g_R = R; g_C = C;
    const NormBwdPlan pl = plan_norm_bwd(R, C);
    ++plans;
    CHECK(pl.cpad % 64 == 0 && pl.cpad >= C && pl.cpad - C < 64);
    CHECK(pl.rows_per_wg >= kNbMinRows);
    CHECK(pl.nwg >= 0 && pl.nwg <= kNbMaxWgs);
    CHECK((pl.nwg == 0) == (R == 0 || C == 0));
    // row ranges: in order, none empty, covering [0, rows) exactly once
    long long next = 0;
    for (int g = 0; g < pl.nwg; ++g) {
      const long long r0 = pl.row_begin(g), r1 = pl.row_end(g, R);
      CHECK(r0 == next && r1 > r0 && r1 - r0 <= pl.rows_per_wg && r1 <= R);
      next = r1;
    }
    if (pl.nwg > 0) CHECK(next == R);
    // regions back to back from 0, inside the reported bytes
    const size_t floats = pl.ws_bytes / sizeof(float);
    CHECK(pl.ws_bytes % sizeof(float) == 0);
    size_t prev_end = 0;
    for (int g = 0; g < pl.nwg; ++g)
      for (int w = 0; w < 2; ++w) {
        const size_t off = pl.part_offset(g, w);
        CHECK(off == prev_end && off + pl.cpad <= floats);
        prev_end = off + pl.cpad;
      }
    CHECK(prev_end == floats);
    // reduce ranges: contiguous, in order, covering [0, nwg) exactly once
    int at = 0;
    for (int r = 0; r < kNbRanges; ++r) {
      CHECK(pl.range_begin(r) == at && pl.range_end(r) >= at);
      CHECK(pl.range_end(r) - pl.range_begin(r) <= pl.per_range);
      at = pl.range_end(r);
    }
    CHECK(at == pl.nwg);
    // the documented bound: 8 cpad min(2048, rows / 4 + 1)
    const long long wgs = R / 4 + 1 < kNbMaxWgs ? R / 4 + 1 : kNbMaxWgs;
    CHECK(pl.ws_bytes <= static_cast<size_t>(8) * pl.cpad * wgs);
  }
  std::printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}

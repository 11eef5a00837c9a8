// Stand-alone check of the conv1d backward's host plan
// (videomamba_amd/csrc/vm_conv_bwd_plan.h): walks plan_conv_bwd() over a grid of shapes and
// exits non-zero unless the time tiles cover [0, seqlen) exactly once with none empty, every
// tile's walk fits eight 8-row loads, every (part, slot) region lies inside the reported size
// without overlapping the next, the reduce ranges cover the parts exactly once in order, and
// the size respects the documented bound.  Built and run by tests/test_train_bwd_cpu.py with
// -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>
#include <vector>

#include "vm_conv_bwd_plan.h"

using namespace vm;

static long g_fail = 0;
static int g_B, g_D, g_L, g_W;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) {                                                                          \
      if (g_fail++ < 20)                                                                    \
        std::fprintf(stderr, "line %d: %s  [B=%d D=%d L=%d W=%d]\n", __LINE__, #cond, g_B,  \
                     g_D, g_L, g_W);                                                        \
    }                                                                                       \
  } while (0)

int main() {
  const int Bs[] = {0, 1, 2, 3, 8, 17, 32, 72};
  const int Ds[] = {0, 1, 8, 63, 64, 65, 136, 1152, 1536};
  const int Ls[] = {0, 1, 3, 4, 5, 60, 61, 62, 63, 64, 65, 122, 123, 150, 1569, 12545};
  const int Ws[] = {1, 2, 3, 4};
  long plans = 0;
  for (int B : Bs) for (int D : Ds) for (int L : Ls) for (int W : Ws) {
    g_B = B; g_D = D; g_L = L; g_W = W;
    const ConvBwdPlan pl = plan_conv_bwd(B, D, L, W);
    ++plans;
    CHECK(kCbWalk == 64 && kCbWalk % 8 == 0 && kCbTT > kCbWM);
    CHECK(pl.slots == W + 1);
    CHECK(pl.dpad % kCbLanes == 0 && pl.dpad >= D && pl.dpad - D < kCbLanes);
    // tiles: in order, none empty, none longer than kCbTT, covering [0, L) exactly once
    CHECK((pl.tiles == 0) == (L == 0));
    std::vector<int> seen(L, 0);
    int next = 0;
    for (int i = 0; i < pl.tiles; ++i) {
      const int t0 = pl.tile_begin(i), t1 = pl.tile_end(i, L);
      CHECK(t0 == next && t1 > t0 && t1 - t0 <= kCbTT && t1 <= L);
      CHECK(t1 - t0 + kCbWM - 1 <= kCbWalk);  // the walk: the tile plus the look-ahead
      CHECK(i == 0 || t0 >= kCbWM - 1);       // the history rows of a later tile are rows of x
      for (int t = t0; t < t1 && t < L; ++t) ++seen[t];
      next = t1;
    }
    CHECK(next == L);
    for (int t = 0; t < L; ++t) CHECK(seen[t] == 1);
    // parts and their regions
    CHECK(pl.parts == (D > 0 ? static_cast<long long>(B) * pl.tiles : 0));
    const size_t floats = pl.ws_bytes / sizeof(float);
    CHECK(pl.ws_bytes % sizeof(float) == 0);
    CHECK((pl.ws_bytes == 0) == (B == 0 || D == 0 || L == 0));
    size_t prev_end = 0;
    for (long long p = 0; p < pl.parts; ++p) {
      for (int s = 0; s < pl.slots; ++s) {
        const size_t off = pl.part_offset(p, s);
        CHECK(off + pl.dpad <= floats);
        CHECK(off == prev_end);  // back to back from 0: disjoint, in order
        prev_end = off + pl.dpad;
      }
    }
    if (pl.parts > 0) CHECK(pl.part_offset(pl.parts - 1, pl.slots - 1) + pl.dpad == floats);
    // reduce ranges: contiguous, in order, covering [0, parts) exactly once
    long long at = 0;
    for (int r = 0; r < kCbRanges; ++r) {
      CHECK(pl.range_begin(r) == at && pl.range_end(r) >= pl.range_begin(r));
      CHECK(pl.range_end(r) - pl.range_begin(r) <= pl.per_range);
      at = pl.range_end(r);
    }
    CHECK(at == pl.parts);
    // the documented bound
    const size_t bound = static_cast<size_t>(20) * B * pl.dpad * (L / kCbTT + 1);
    CHECK(pl.ws_bytes <= bound);
  }
  std::printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}

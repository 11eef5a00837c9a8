// Stand-alone check of the selective scan backward's host plan
// (videomamba_amd/csrc/vm_scan_bwd_plan.h): walks plan_scan_bwd() over a grid of shapes and
// exits non-zero unless every plan's workspace regions are disjoint and inside the reported
// size, the size respects the documented bound, and the chunks tile the sequence with none
// empty.  Built and run by tests/test_scan_bwd_cpu.py with -fsanitize=address,undefined;
// needs no GPU and no HIP.
#include <cstdio>

#include "vm_scan_bwd_plan.h"

using namespace vm;

static long g_fail = 0;
static int g_B, g_D, g_L;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      if (g_fail++ < 20)                                                                   \
        std::fprintf(stderr, "line %d: %s  [B=%d D=%d L=%d]\n", __LINE__, #cond, g_B, g_D, \
                     g_L);                                                                 \
    }                                                                                      \
  } while (0)

int main() {
  const int Bs[] = {0, 1, 2, 3, 8, 32, 72, 336};
  const int Ds[] = {0, 1, 63, 64, 65, 136, 1152, 1536};
  const int Ls[] = {0, 1, 5, 7, 8, 9, 16, 17, 24, 33, 150, 1569, 3137, 12545};
  long plans = 0;
  for (int B : Bs) for (int D : Ds) for (int L : Ls) {
    g_B = B; g_D = D; g_L = L;
    const ScanBwdPlan pl = plan_scan_bwd(B, D, L);
    ++plans;
    const size_t b = B, l = L;
    // geometry: whole 64-lane groups cover the channels
    CHECK(pl.groups * kBwdLanes == pl.dpad && pl.dpad >= D && pl.dpad - D < kBwdLanes);
    CHECK(pl.T == kBwdT && pl.T >= 8);
    // the chunks tile [0, L) in order, none empty, none longer than T
    CHECK((pl.nchunks == 0) == (L == 0));
    int next = 0;
    for (int c = 0; c < pl.nchunks; ++c) {
      const int t0 = pl.chunk_begin(c), t1 = pl.chunk_end(c, L);
      CHECK(t0 == next && t1 > t0 && t1 - t0 <= pl.T && t1 <= L);
      if (c + 1 < pl.nchunks) CHECK(t1 - t0 == pl.T);  // sweep 1 runs whole chunks only
      next = t1;
    }
    CHECK(next == L);
    // regions in order, disjoint, inside the reported bytes
    const size_t rows = b * pl.dpad;
    CHECK(pl.ckpt == 0);
    CHECK(pl.ckpt + pl.ckpt_floats(B) <= pl.bc);
    CHECK(pl.bc + pl.bc_floats(B, L) <= pl.pa);
    CHECK(pl.pa + rows * kBwdN <= pl.pd);
    CHECK(pl.pd + rows <= pl.pb);
    CHECK((pl.pb + rows) * sizeof(float) <= pl.ws_bytes);
    // the largest index each kernel forms lies inside its region
    if (B > 0 && D > 0 && pl.nchunks > 1) {
      const size_t last_ck = ((b - 1) * (pl.nchunks - 1) + (pl.nchunks - 2)) * pl.groups +
                             (pl.groups - 1);
      CHECK((last_ck * kBwdN + (kBwdN - 1)) * kBwdLanes + (kBwdLanes - 1) < pl.ckpt_floats(B));
    }
    if (B > 0 && D > 0 && L > 0) {
      const size_t last_bc = (((b - 1) * pl.groups + (pl.groups - 1)) * l + (l - 1)) * 2 * kBwdN +
                             (2 * kBwdN - 1);
      CHECK(last_bc < pl.bc_floats(B, L));
    }
    // the documented bound: no per-step state dump
    const size_t bound = 12 * b * l * pl.dpad + 4 * b * pl.dpad * (kBwdN + 2) + 4096;
    CHECK(pl.ws_bytes <= bound);
    CHECK((pl.ws_bytes == 0) == (B == 0 || D == 0));
  }
  std::printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}

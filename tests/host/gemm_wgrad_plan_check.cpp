// Stand-alone check of the projection GEMM weight gradient's host plan
// (videomamba_amd/csrc/vm_gemm_wgrad_plan.h): walks plan_linear_wgrad() over a grid of
// (m, n, k) and exits non-zero unless the slices tile [0, m) exactly once in order with none
// empty, the output tiles cover (n, k) exactly once, every slice's partial tile lies inside
// the reported workspace, workspace_bytes equals the size query's and respects the documented
// bound and never shrinks as m grows, the LDS size fits 160 KiB, the plan's inputs hold no CU
// count, and the refusals come in the documented order.  Built and run by
// tests/test_linear_bwd_cpu.py with -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>
#include <type_traits>
#include <vector>

#include "vm_gemm_wgrad_plan.h"

using namespace vm;

static long g_fail = 0;
static int g_m, g_n, g_k;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (g_fail++ < 20)                                                                     \
        std::fprintf(stderr, "line %d: %s  [m=%d n=%d k=%d]\n", __LINE__, #cond, g_m, g_n,  \
                     g_k);                                                                   \
    }                                                                                        \
  } while (0)

// The plan takes (m, n, k), strides, flags and the caller's workspace size: 3 ints, 4 long
// longs and 6 bools.  A CU count (or any other device property) would be one more member.
static_assert(std::is_standard_layout<WgradPlanIn>::value, "plain inputs");
static_assert(sizeof(WgradPlanIn) <= 3 * sizeof(int) + 4 + 3 * sizeof(long long) + 8 +
                                         sizeof(long long),
              "WgradPlanIn grew: a device-dependent input would break bit-reproducibility");

static WgradPlanIn base(int m, int n, int k) {
  WgradPlanIn in{};
  in.m = m; in.n = n; in.k = k;
  in.lddy = n; in.ldx = k; in.lddw = k;
  in.bf16 = true; in.dw_dtype_ok = true;
  in.dy_al = in.x_al = in.dw_al = in.ws_al = true;
  in.workspace_bytes = plan_linear_wgrad_shape(m, n, k).workspace_bytes;
  return in;
}

int main() {
  const int Ms[] = {0, 1, 31, 32, 33, 65, 255, 256, 257, 511, 513, 773, 1024, 1025, 1537, 3144,
                    12552, 12553, 50208, 200000, 1000000};
  const int Ns[] = {8, 72, 128, 136, 192, 384, 576, 768, 1152, 2304, 3072};
  const int Ks[] = {64, 128, 192, 384, 576, 768, 1152, 1536, 2304};
  long plans = 0;
  for (int n : Ns) for (int k : Ks) {
    long long prev_ws = 0;
    for (int m : Ms) {
      g_m = m; g_n = n; g_k = k;
      WgradPlanIn in = base(m, n, k);
      if (static_cast<long long>(m) * (n > k ? n : k) * 2 >= kWg2G) continue;
      const WgradPlan pl = plan_linear_wgrad(in);
      ++plans;
      CHECK(pl.why == WgradWhy::kOk);
      CHECK(pl.empty == (m == 0));
      // slices: in order, none empty, [0, m) exactly once, whole stages
      CHECK(pl.slice_rows >= kWgMinSliceRows && pl.slice_rows % kWgStageRows == 0);
      CHECK(pl.slices <= pl.max_slices && pl.max_slices >= kWgMinSlices);
      long long next = 0;
      for (int s = 0; s < pl.slices; ++s) {
        const long long r0 = pl.row_begin(s), r1 = pl.row_end(s, m);
        CHECK(r0 == next && r1 > r0 && r1 - r0 <= pl.slice_rows && r1 <= m);
        next = r1;
      }
      CHECK(next == m);
      CHECK(pl.gz == (m == 0 ? 0u : static_cast<unsigned>(pl.slices)));
      // tiles: (n, k) exactly once
      CHECK(pl.gx == static_cast<unsigned>(pl.tiles_k) && pl.gy == static_cast<unsigned>(pl.tiles_n));
      std::vector<unsigned char> seen(static_cast<size_t>(n) * k, 0);
      for (int tn = 0; tn < pl.tiles_n; ++tn)
        for (int tk = 0; tk < pl.tiles_k; ++tk)
          for (int r = tn * kWgTileN; r < (tn + 1) * kWgTileN && r < n; ++r)
            for (int c = tk * kWgTileK; c < (tk + 1) * kWgTileK && c < k; ++c)
              ++seen[static_cast<size_t>(r) * k + c];
      bool once = true;
      for (unsigned char v : seen) once = once && v == 1;
      CHECK(once);
      // partial tiles back to back inside the workspace; the reduce kernel covers dw
      CHECK(pl.workspace_bytes % 4 == 0);
      for (int s = 0; s < pl.slices; ++s) {
        CHECK(pl.part_offset(s, n, k) == static_cast<size_t>(s) * n * k);
        CHECK((pl.part_offset(s, n, k) + static_cast<size_t>(n) * k) * 4 <=
              static_cast<size_t>(pl.workspace_bytes));
      }
      CHECK(static_cast<long long>(pl.rgx) * pl.rblock >= static_cast<long long>(n) * (k / 4));
      CHECK(static_cast<long long>(pl.rgx - 1) * pl.rblock < static_cast<long long>(n) * (k / 4));
      // the query, the bound, monotone in m
      CHECK(pl.workspace_bytes == plan_linear_wgrad_shape(m, n, k).workspace_bytes);
      CHECK(pl.workspace_bytes <= wgrad_ws_bound(n, k));
      CHECK(pl.workspace_bytes <= 16ll * n * k + (32ll << 20));
      CHECK(pl.workspace_bytes >= prev_ws);
      prev_ws = pl.workspace_bytes;
      CHECK(pl.lds == kWgLdsBytes && pl.lds <= 160u * 1024u && pl.block == kWgThreads);
      CHECK(pl.gz <= 65535u && pl.gy <= 65535u);

      // refusal order: dtype, shape, strides, alignment, 2 GB, workspace
      WgradPlanIn bad = in;
      bad.bf16 = false; bad.n = n + 1; bad.lddy = 4; bad.dy_al = false; bad.workspace_bytes = -1;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kDtype);
      bad.bf16 = true; bad.dw_dtype_ok = false;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kDtype);
      bad.dw_dtype_ok = true;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kShape);
      bad.n = n; bad.k = k + 32;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kShape);
      bad.k = k;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kStrides);
      bad.lddy = n; bad.ldx = k + 4;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kStrides);
      bad.ldx = k; bad.lddw = k - 8;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kStrides);
      bad.lddw = k;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kAlign);
      bad.dy_al = true; bad.ws_al = false;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kAlign);
      bad.ws_al = true;
      if (m > 0) {
        const long long big = kWg2G / 2 / m + 8;
        WgradPlanIn far = bad;
        far.ldx = (big + 7) / 8 * 8;
        if (far.ldx >= k) CHECK(plan_linear_wgrad(far).why == WgradWhy::kPast2GB);
      }
      if (pl.workspace_bytes > 0) {
        CHECK(plan_linear_wgrad(bad).why == WgradWhy::kWorkspace);
        bad.workspace_bytes = pl.workspace_bytes - 1;
        CHECK(plan_linear_wgrad(bad).why == WgradWhy::kWorkspace);
        CHECK(plan_linear_wgrad(bad).gz == 0 && plan_linear_wgrad(bad).rgx == 0);
      }
      bad.workspace_bytes = pl.workspace_bytes + 4096;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kOk);
      bad.lddy = n + 8; bad.ldx = k + 64; bad.lddw = k + 8;
      CHECK(plan_linear_wgrad(bad).why == WgradWhy::kOk);
    }
  }
  std::printf("%ld plans, %ld failures\n", plans, g_fail);
  return g_fail ? 1 : 0;
}

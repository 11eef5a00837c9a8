// Stand-alone check of the projection GEMM's host plan (videomamba_amd/csrc/vm_gemm_plan.h):
// walks plan_linear() and plan_linear_add_norm() over a grid of shapes and exits non-zero
// unless every plan picks the form the rules below give and is self-consistent, and the fits
// queries (linear_fits, linear_add_norm_fits, linear_fn_fits) answer as the rules do.  The rules are
// written out a second time here, as vm_linear_fwd_form and vm_linear_add_norm_fwd had them
// before the plan (literal numbers, not the header's constants).  Built and run by
// tests/test_api_cpu.py with -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "vm_gemm_plan.h"
#include "vm_gemm_wgrad_plan.h"

using namespace vm;

static long g_fail = 0;
static const GemmPlanIn* g_in = nullptr;
#define CHECK(cond)                                                                            \
  do {                                                                                         \
    if (!(cond)) {                                                                             \
      if (g_fail++ < 20)                                                                       \
        std::fprintf(stderr,                                                                   \
                     "line %d: %s  [m=%d n=%d k=%d ldx=%lld ldw=%lld ldo=%lld ldr=%lld "       \
                     "ldh=%lld bias=%d bf16=%d form=%d al=%d%d%d%d%d%d cus=%d cb=%lld]\n",     \
                     __LINE__, #cond, g_in->m, g_in->n, g_in->k, g_in->ldx, g_in->ldw,         \
                     g_in->ldo, g_in->ldr, g_in->ldh, g_in->has_bias, g_in->bf16, g_in->form,  \
                     g_in->x_al, g_in->w_al, g_in->o_al, g_in->r_al, g_in->nw_al, g_in->hn_al, \
                     g_in->cus, g_in->counter_bytes);                                          \
    }                                                                                          \
  } while (0)

constexpr size_t kLdsPerCu = 160 * 1024;  // MI355X: 160 KB of LDS per CU
constexpr long long k2G = 1ll << 31;

static long g_seen[kGemmForms];
static long g_plans = 0;
static long g_fn_fits = 0;

// ---------------------------------------------------------------- the rules, written out
static bool k_in_list(int k) {
  switch (k / 64) {
    case 3: case 6: case 9: case 12: case 18: case 24: return true;
    default: return false;
  }
}
// the persistent tile width: 0 none
static int want_tile_bn(const GemmPlanIn& in) {
  if (in.k % 64 != 0 || !k_in_list(in.k)) return 0;
  const int n = in.n;
  const int bn = (n >= 1024 && n % 256 == 0) ? 256 : (n % 192 == 0 ? 192 : (n % 256 == 0 ? 256 : 0));
  if (!bn) return 0;
  if (256ll * in.ldx * 2 >= k2G || 256ll * in.ldo * 2 >= k2G || 1ll * bn * in.ldw * 2 >= k2G) return 0;
  return bn;
}
static long long want_tiles(const GemmPlanIn& in, int bn) {
  return ((1ll * in.m + 255) / 256) * (in.n / bn);
}
static GemmForm want_linear(const GemmPlanIn& in, GemmWhy& why) {
  why = GemmWhy::kOk;
  if (in.form < 0 || in.form > 2) return why = GemmWhy::kFormArg, GemmForm::kNone;
  if (!in.bf16 || in.m < 0 || in.n < 1 || in.k < 64 || in.n % 8 || in.k % 64 || in.ldx < in.k ||
      in.ldw < in.k || in.ldo < in.n || in.ldx % 8 || in.ldw % 8 || in.ldo % 8 || !in.x_al ||
      !in.w_al || !in.o_al || 1ll * in.n * in.ldw * 2 >= k2G)
    return why = GemmWhy::kShape, GemmForm::kNone;
  if (!k_in_list(in.k)) return why = GemmWhy::kK, GemmForm::kNone;
  if (in.m == 0) return GemmForm::kEmpty;
  const int bn = in.has_bias ? 0 : want_tile_bn(in);
  if (in.form == 2 && !bn) return why = GemmWhy::kTileShape, GemmForm::kNone;
  if (in.form != 1 && bn) {
    const int wgs = in.cus / 8 * 8;
    if (in.form == 2 && wgs < 8) return why = GemmWhy::kTileCus, GemmForm::kNone;
    if (wgs >= 8 && (in.form == 2 || 2 * want_tiles(in, bn) >= 3ll * wgs))
      return bn == 256 ? GemmForm::kTile256 : GemmForm::kTile192;
  }
  if (1ll * in.m * in.ldx * 2 >= k2G) return why = GemmWhy::kXPast2GB, GemmForm::kNone;
  return in.n >= 1024 ? GemmForm::kDma128x128 : GemmForm::kDma128x64;
}

static long long want_counter_bytes(int m) { return m <= 0 ? 0 : 4 * (16 + 2 * ((1ll * m + 127) / 128)); }

static bool norm_pair(int n, int k) {
  return (n == 192 && k == 384) || (n == 384 && k == 768) || (n == 576 && k == 1152);
}

static GemmForm want_add_norm(const GemmPlanIn& in, GemmWhy& why) {
  why = GemmWhy::kOk;
  if (in.m < 0 || in.n < 4 || in.n > 1024 || in.n % 8 || in.k < 64 || in.k % 64 || in.ldx < in.k ||
      in.ldw < in.k || in.ldo < in.n || in.ldr < in.n || in.ldh < in.n || in.ldx % 8 || in.ldw % 8 ||
      in.ldo % 8 || in.ldr % 4 || in.ldh % 4 || !in.x_al || !in.w_al || !in.o_al || !in.r_al ||
      !in.nw_al || !in.hn_al || 1ll * in.n * in.ldw * 2 >= k2G ||
      in.counter_bytes < want_counter_bytes(in.m))
    return why = GemmWhy::kNormShape, GemmForm::kNone;
  if (!k_in_list(in.k)) return why = GemmWhy::kNormK, GemmForm::kNone;
  if (in.m == 0) return GemmForm::kEmpty;
  // one launch when the whole 128 x 64-tile grid is co-resident at one workgroup per CU.  The
  // one condition the entry did not have before the plan: its x and h each go through one
  // buffer of m rows (31-bit offsets in the kernel); rows past that take the later forms.
  const long long nwg = ((1ll * in.m + 127) / 128) * ((in.n + 63) / 64);
  if (in.cus > 0 && nwg <= in.cus && 1ll * in.m * in.ldx * 2 < k2G && 1ll * in.m * in.ldo * 2 < k2G)
    return GemmForm::kDmaNorm;
  const int bn = want_tile_bn(in);
  const int wgs = in.cus / 8 * 8;
  if (bn && bn == 192 && norm_pair(in.n, in.k) && wgs >= 8 && 2 * want_tiles(in, bn) >= 3ll * wgs)
    return GemmForm::kTileNorm;
  if (in.ldo != in.n || in.ldr != in.n || in.ldh != in.n) return why = GemmWhy::kNormStrides, GemmForm::kNone;
  return GemmForm::kTwoLaunch;
}

// ---------------------------------------------------------------- what every plan must hold
static void check_common(const GemmPlanIn& in, const GemmPlan& pl) {
  ++g_plans;
  ++g_seen[static_cast<int>(pl.form)];
  CHECK((pl.why == GemmWhy::kOk) == (pl.form != GemmForm::kNone));
  const bool launches = pl.form != GemmForm::kNone && pl.form != GemmForm::kEmpty &&
                        pl.form != GemmForm::kTwoLaunch;
  CHECK((pl.gx != 0) == launches);
  if (!launches) return;
  CHECK(in.m > 0 && pl.reads_cus);
  CHECK(pl.NK * 64 == in.k && k_in_list(pl.NK * 64));  // an instantiated K-step count
  CHECK(pl.lds <= kLdsPerCu && pl.block == 512);
  const bool tile = pl.form == GemmForm::kTile256 || pl.form == GemmForm::kTile192 ||
                    pl.form == GemmForm::kTileNorm;
  if (tile) {
    CHECK(pl.bn == (pl.form == GemmForm::kTile256 ? 256 : 192));
    CHECK(in.n % pl.bn == 0 && pl.ntn == in.n / pl.bn);
    CHECK(pl.tiles == ((1ll * in.m + 255) / 256) * (in.n / pl.bn));
    CHECK(1ll * pl.tpx * 8 >= pl.tiles);
    CHECK(pl.wgs % 8 == 0 && pl.wgs >= 8 && pl.wgs <= in.cus);
    CHECK(pl.gx == static_cast<unsigned>(pl.wgs) && pl.gy == 1);
    CHECK(pl.lds == 2u * (256 + pl.bn) * 128);
    CHECK(256 * in.ldx * 2 < k2G && 256 * in.ldo * 2 < k2G && pl.bn * in.ldw * 2 < k2G);
    CHECK(!in.has_bias);
    if (pl.form == GemmForm::kTileNorm) {
      CHECK(pl.tpx % pl.ntn == 0);
      CHECK(norm_pair(in.n, in.k));
      CHECK(pl.NC == (in.n + 255) / 256 && pl.NC >= 1 && pl.NC <= 3);
      CHECK(pl.NK % 2 == 0);  // the NORM instances need an even K-step count
    }
  } else {
    const int bm = 128, bn = pl.form == GemmForm::kDma128x128 ? 128 : 64;
    const int nbuf = pl.form == GemmForm::kDma128x128 ? 2 : 3;
    CHECK(pl.bn == bn);
    // the grid covers m x n with no idle tile row or column
    CHECK(1ll * pl.gx * bm >= in.m && 1ll * (pl.gx - 1) * bm < in.m);
    CHECK(1ll * pl.gy * bn >= in.n && 1ll * (pl.gy - 1) * bn < in.n);
    CHECK(pl.gy <= 65535);
    CHECK(in.m * in.ldx * 2 < k2G && in.n * in.ldw * 2 < k2G);
    if (pl.form == GemmForm::kDmaNorm) {
      // the hand-off's condition: every workgroup resident, one per CU
      CHECK(1ll * pl.gx * pl.gy <= in.cus);
      CHECK(pl.lds == 96u * 1024 && 2 * pl.lds > kLdsPerCu);
      CHECK(pl.lds >= static_cast<size_t>(nbuf) * (bm + bn) * 128);
      CHECK(in.m * in.ldo * 2 < k2G);
      CHECK(in.n <= 1024);
    } else {
      CHECK(pl.lds == static_cast<size_t>(nbuf) * (bm + bn) * 128);
    }
  }
}

static void check_linear(const GemmPlanIn& in) {
  g_in = &in;
  const GemmPlan pl = plan_linear(in);
  GemmWhy why;
  const GemmForm want = want_linear(in, why);
  CHECK(pl.form == want);
  CHECK(pl.why == why);
  check_common(in, pl);
  // vm_linear_fits: the plan's own answer, from the input the entries build
  CHECK(linear_fits(in) == (want != GemmForm::kNone));
  const GemmPlanIn built = gemm_linear_in(in.m, in.n, in.k, in.ldx, in.ldw, in.ldo, in.has_bias,
                                          in.bf16, in.form, in.x_al, in.w_al, in.o_al);
  CHECK(built.cus == 0 && !built.dgrad);
  GemmPlanIn on = built;
  on.cus = in.cus;
  CHECK(linear_fits(on) == (want != GemmForm::kNone) && plan_linear(on).form == want);
}

// vm_linear_fn_fits as kernels.linear_fn's gate had it before the query: m >= 1, k one of the
// forward's reduction lengths, n one of dgrad's, m rows of the wider operand under 2^31 bytes
static bool want_linear_fn(int m, int n, int k) {
  return m >= 1 && k % 64 == 0 && k_in_list(k) && n % 64 == 0 && (k_in_list(n) || n == 2304) &&
         2ll * m * (n > k ? n : k) < k2G;
}

static void check_add_norm(const GemmPlanIn& in) {
  g_in = &in;
  const GemmPlan pl = plan_linear_add_norm(in);
  GemmWhy why;
  const GemmForm want = want_add_norm(in, why);
  CHECK(pl.form == want);
  CHECK(pl.why == why);
  CHECK(pl.counter_bytes == want_counter_bytes(in.m));
  CHECK(pl.counter_bytes == gemm_counter_bytes(in.m));
  check_common(in, pl);
  // vm_linear_add_norm_fits: the plan's own answer, from the input the entry builds
  CHECK(linear_add_norm_fits(in) == (want != GemmForm::kNone));
  GemmPlanIn built = gemm_add_norm_in(in.m, in.n, in.k, in.ldx, in.ldw, in.ldo, in.ldr, in.ldh,
                                      in.x_al, in.w_al, in.o_al, in.r_al, in.nw_al, in.hn_al,
                                      in.counter_bytes);
  CHECK(built.cus == 0 && built.bf16 && !built.has_bias && built.form == 0);
  built.cus = in.cus;
  CHECK(plan_linear_add_norm(built).form == want);
  if (pl.form == GemmForm::kTwoLaunch)
    CHECK(in.ldo == in.n && in.ldr == in.n && in.ldh == in.n);
  // the persistent test is vm_linear_fwd's: past the one-launch form, the fused entry runs
  // the persistent NORM kernel exactly where form 0 picks the persistent kernel on the same
  // operands (and a NORM instance exists)
  if (pl.form == GemmForm::kTileNorm || pl.form == GemmForm::kTwoLaunch ||
      pl.why == GemmWhy::kNormStrides) {
    GemmPlanIn lin = in;
    lin.form = 0; lin.has_bias = false; lin.bf16 = true;
    const GemmPlan lp = plan_linear(lin);
    const bool persistent = lp.form == GemmForm::kTile256 || lp.form == GemmForm::kTile192;
    CHECK((pl.form == GemmForm::kTileNorm) ==
          (persistent && lp.bn == 192 && norm_pair(in.n, in.k)));
    if (pl.form == GemmForm::kTileNorm)
      CHECK(lp.tiles == pl.tiles && lp.wgs == pl.wgs && lp.ntn == pl.ntn);
  }
}

// ---------------------------------------------------------------- the walk
static long long first_past(long long rows) {  // the first multiple of 8 with rows * ld * 2 >= 2^31
  const long long ld = ((1ll << 30) + rows - 1) / rows;
  return (ld + 7) / 8 * 8;
}

int main() {
  const int ms[] = {0, 1, 127, 128, 129, 255, 256, 257, 3144, 12552, 40000, 1408512, 0x7fffffff};
  const int ns[] = {8, 64, 136, 192, 200, 384, 576, 768, 1024, 1032, 1536, 2304};
  const int cus[] = {0, 7, 8, 64, 256, 304};
  std::vector<int> ks = {0, 96};
  for (int k = 64; k <= 2048; k += 64) ks.push_back(k);

  auto base = [](int m, int n, int k, int cu) {
    GemmPlanIn in{};
    in.m = m; in.n = n; in.k = k; in.ldx = k; in.ldw = k; in.ldo = n; in.ldr = n; in.ldh = n;
    in.bf16 = true;
    in.x_al = in.w_al = in.o_al = in.r_al = in.nw_al = in.hn_al = true;
    in.cus = cu;
    in.counter_bytes = want_counter_bytes(m);
    return in;
  };

  for (int m : ms)
    for (int n : ns)
      for (int k : ks)
        for (int cu : cus) {
          // ---- vm_linear_fwd_form: contiguous operands, every form and bias
          for (int form = -1; form <= 3; ++form)
            for (int bias = 0; bias < 2; ++bias) {
              GemmPlanIn in = base(m, n, k, cu);
              in.form = form; in.has_bias = bias != 0;
              check_linear(in);
            }
          // ---- vm_linear_add_norm_fwd: contiguous operands
          check_add_norm(base(m, n, k, cu));
          // ---- vm_linear_fn_fits: forward, dgrad and wgrad of one shape
          {
            const GemmPlanIn in = base(m, n, k, cu);
            g_in = &in;
            CHECK(linear_fn_fits(m, n, k, cu) == want_linear_fn(m, n, k));
            CHECK(linear_fn_fits(m, k, n, cu) == want_linear_fn(m, k, n));
            g_fn_fits += linear_fn_fits(m, n, k, cu) + linear_fn_fits(m, k, n, cu);
          }
          if (k != 0 && k != 96 && k != 576 && k != 1152 && k != 384 && k != 640) continue;
          // ---- leading dimensions: padded, and on both sides of every 2^31-byte limit
          const long long rows_m = m > 0 ? m : 1;
          const long long ldxs[] = {k + 8ll, k + 4ll, first_past(rows_m) - 8, first_past(rows_m),
                                    first_past(256) - 8, first_past(256)};
          const long long ldws[] = {k + 8ll, k + 4ll, first_past(n) - 8, first_past(n),
                                    first_past(192) - 8, first_past(192), first_past(256)};
          const long long ldos[] = {n + 8ll, n + 4ll, first_past(rows_m) - 8, first_past(rows_m),
                                    first_past(256) - 8, first_past(256)};
          for (int form = 0; form <= 2; ++form) {
            for (long long ld : ldxs) {
              GemmPlanIn in = base(m, n, k, cu);
              in.form = form; in.ldx = ld;
              check_linear(in);
              if (form == 0) check_add_norm(in);
            }
            for (long long ld : ldws) {
              GemmPlanIn in = base(m, n, k, cu);
              in.form = form; in.ldw = ld;
              check_linear(in);
              if (form == 0) check_add_norm(in);
            }
            for (long long ld : ldos) {
              GemmPlanIn in = base(m, n, k, cu);
              in.form = form; in.ldo = ld;
              check_linear(in);
              if (form == 0) check_add_norm(in);
            }
            // ---- each alignment flag off once, another dtype
            for (int a = 0; a < 4; ++a) {
              GemmPlanIn in = base(m, n, k, cu);
              in.form = form;
              if (a == 0) in.x_al = false;
              if (a == 1) in.w_al = false;
              if (a == 2) in.o_al = false;
              if (a == 3) in.bf16 = false;
              check_linear(in);
            }
          }
          for (long long ld : {n + 4ll, n + 8ll, n + 2ll, n - 4ll}) {
            GemmPlanIn in = base(m, n, k, cu);
            in.ldr = ld;
            check_add_norm(in);
            in = base(m, n, k, cu);
            in.ldh = ld;
            check_add_norm(in);
          }
          for (int a = 0; a < 6; ++a) {
            GemmPlanIn in = base(m, n, k, cu);
            if (a == 0) in.x_al = false;
            if (a == 1) in.w_al = false;
            if (a == 2) in.o_al = false;
            if (a == 3) in.r_al = false;
            if (a == 4) in.nw_al = false;
            if (a == 5) in.hn_al = false;
            check_add_norm(in);
          }
          for (long long d : {-1ll, 1ll << 20}) {  // counter bytes one short, and plenty
            GemmPlanIn in = base(m, n, k, cu);
            in.counter_bytes += d;
            check_add_norm(in);
          }
        }

  // the list macro, the predicate and the rules agree on every k
  for (int k = -128; k <= 4096; ++k) {
    GemmPlanIn in{};
    g_in = &in;
    in.k = k;
    CHECK(gemm_k_ok(k) == (k > 0 && k % 64 == 0 && k_in_list(k)));
  }
  // every form is reached
  for (int f = 0; f < kGemmForms; ++f) {
    if (!g_seen[f]) {
      std::fprintf(stderr, "form %d never planned\n", f);
      ++g_fail;
    }
  }
  if (!g_fn_fits) {
    std::fprintf(stderr, "vm_linear_fn_fits never answered 1\n");
    ++g_fail;
  }
  std::printf("per form:");
  for (int f = 0; f < kGemmForms; ++f) std::printf(" %ld", g_seen[f]);
  std::printf("\n%ld plans, %ld failures\n", g_plans, g_fail);
  return g_fail ? 1 : 0;
}

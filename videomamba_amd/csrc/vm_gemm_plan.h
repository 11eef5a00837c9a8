// Host-side plan of the projection GEMM (in_proj / out_proj of every layer): which kernel
// form takes a shape, the refusals, the launch geometry and the counter buffer.  Plain C++17,
// no HIP header: vm_linear_fwd_form, vm_linear_add_norm_fwd and their launchers (vm_gemm.hip,
// vm_gemm_tile.hip) read one GemmPlan, the kernels take the K step, the staged row and the
// counter layout from the constants below, and tests/host/gemm_plan_check.cpp walks both
// planners over a grid of shapes on the host.  To add a K, a tile shape or a form, change
// this file and the launch switch of that form.
#pragma once

#include <cstddef>

namespace vm {

// ---------------------------------------------------------------- shared constants
constexpr int kGemmBK = 64;    // K step: bf16 elements of K per staged row
constexpr int kGemmRow = 128;  // bytes per staged row (kGemmBK bf16)

// The unrolled K-step counts (k / kGemmBK) every GEMM kernel is instantiated for; the in_proj
// form of the mixer middle (vm_inproj_conv.hip) runs the same set.
#define VM_GEMM_NK_LIST(X) X(3) X(6) X(9) X(12) X(18) X(24)
constexpr long long gemm_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
constexpr bool gemm_k_ok(int k) {
  if (k <= 0 || k % kGemmBK != 0) return false;
#define VM_GEMM_NK_IS(NKV) if (k / kGemmBK == NKV) return true;
  VM_GEMM_NK_LIST(VM_GEMM_NK_IS)
#undef VM_GEMM_NK_IS
  return false;
}
// vm_linear_dgrad (dx = dy w: the forward kernels with the transposed weight, the reduction
// running over the forward's n) takes the same list plus 36 steps, VideoMamba-M's in_proj
// (n = 2304).  The forward entries and the mixer middle keep VM_GEMM_NK_LIST.
#define VM_GEMM_DGRAD_NK_LIST(X) VM_GEMM_NK_LIST(X) X(36)
constexpr bool gemm_dgrad_k_ok(int k) {
  return gemm_k_ok(k) || (k > 0 && k % kGemmBK == 0 && k / kGemmBK == 36);
}

// LDS-DMA tiles (linear_dma_kernel): bm x bn outputs, nbuf stage buffers of (bm + bn) staged
// rows, 2 * nwm waves.  Wide outputs (n >= kDmaWideMinN: in_proj) take 128 x 128 with two
// buffers (64 KB: two workgroups per CU), narrow ones (out_proj) 128 x 64 with three (72 KB).
struct DmaTile {
  int bm, bn, nbuf, nwm;
  constexpr unsigned threads() const { return 128u * nwm; }
  constexpr size_t lds() const { return static_cast<size_t>(nbuf) * (bm + bn) * kGemmRow; }
};
constexpr DmaTile kDmaWide{128, 128, 2, 4};
constexpr DmaTile kDmaNarrow{128, 64, 3, 4};
constexpr int kDmaWideMinN = 1024;
// The one-launch add + norm form runs the narrow tile; it asks for 96 KB (its stages need
// 72 KB) so that a CU holds one workgroup: the validated one-per-CU form of the hand-off.
constexpr DmaTile kDmaNormTile{128, 64, 3, 4};
constexpr size_t kDmaNormLds = 96 * 1024;
constexpr int kNormMaxN = 1024;  // its phase B holds a row as 4 chunks of 256 columns

// Persistent tiles (gemm_tile_kernel): 256 x 256 (waves 2 x 4) or 256 x 192 (waves 4 x 2),
// two stage buffers, 512 threads, one workgroup per CU on whole XCD runs (multiples of 8).
constexpr int kTileBM = 256;
constexpr int kTileBNWide = 256, kTileBNNarrow = 192;
constexpr unsigned kTileThreads = 512;
constexpr size_t tile_lds(int bn) { return static_cast<size_t>(2) * (kTileBM + bn) * kGemmRow; }
// the persistent kernel runs from 1.5 tiles per CU (twice the tile count >= 3 x CUs): C5's
// in_proj (12,544 rows, 441 tiles) 41.9 -> ~35 us, the C5 chunk 8.55 -> 8.26 ms
constexpr int kTileMinPerCU2 = 3;
// The persistent NORM form (out_proj + the next block's add + RMSNorm) is instantiated for
// the VideoMamba Ti / S / M out_proj: X(n, k), on 256 x 192 tiles.
#define VM_GEMM_TILE_NORM_LIST(X) X(192, 384) X(384, 768) X(576, 1152)

// Counter buffer of vm_linear_add_norm_fwd, in 32-bit words: an error word (+ pad), then two
// counters (producers, consumers) per kCntRows-row tile.
constexpr int kCntHead = 16;
constexpr int kCntRows = 128;
constexpr long long gemm_counter_bytes(int m) {
  return m <= 0 ? 0 : (kCntHead + 2 * gemm_ceil_div(m, kCntRows)) * 4;
}
static_assert(kDmaNormTile.bm == kCntRows, "the one-launch form counts per row tile of its own");
static_assert(kTileBM >= kCntRows, "the persistent NORM form counts per 256-row block");

// ---------------------------------------------------------------- the plan
enum class GemmForm {
  kNone,        // refused: see GemmPlan::why
  kEmpty,       // m == 0: VM_OK, nothing launches
  kDma128x128,  // linear_dma_kernel on kDmaWide
  kDma128x64,   // linear_dma_kernel on kDmaNarrow
  kTile256,     // gemm_tile_kernel, 256 x 256
  kTile192,     // gemm_tile_kernel, 256 x 192
  kDmaNorm,     // linear_dma_kernel<NORM> on kDmaNormTile: one launch, whole grid co-resident
  kTileNorm,    // gemm_tile_kernel<NORM>, 256 x 192
  kTwoLaunch,   // vm_linear_fwd + vm_add_norm_fwd
};
constexpr int kGemmForms = 9;

enum class GemmWhy {
  kOk,
  kFormArg,      // form outside 0 .. 2
  kShape,        // vm_linear_fwd's shape and alignment block
  kK,            // k outside the list (vm_linear_fwd)
  kTileShape,    // form 2 asked of a shape without a persistent tile
  kTileCus,      // form 2 on fewer than 8 CUs (or the query failed)
  kXPast2GB,     // the LDS-DMA form addresses x through one 31-bit buffer
  kNormShape,    // vm_linear_add_norm_fwd's shape block (counter_bytes included)
  kNormK,        // k outside the list (vm_linear_add_norm_fwd)
  kNormStrides,  // the two separate launches need contiguous h / residual / hn rows
};

struct GemmPlanIn {
  int m, n, k;
  long long ldx, ldw, ldo;  // row strides, in elements
  bool has_bias;
  bool bf16;                // dtype == VM_DTYPE_BF16
  int form;                 // 0 by shape, 1 LDS-DMA tiles, 2 persistent
  bool x_al, w_al, o_al;    // 16-byte alignment of x, w, out / h
  int cus;                  // CU count of the launch device, 0 when unknown
  // vm_linear_add_norm_fwd only
  long long ldr, ldh;
  bool r_al, nw_al, hn_al;  // residual, norm weight, hn
  long long counter_bytes;
  // vm_linear_dgrad only: K from VM_GEMM_DGRAD_NK_LIST
  bool dgrad;
};

struct GemmPlan {
  GemmForm form;
  GemmWhy why;
  int bn;                  // tile width
  int NK, NC;              // template selectors: k / 64; NORM: 256-column chunks of a row
  unsigned gx, gy, block;  // gx == 0: not launched
  size_t lds;              // dynamic LDS bytes
  int tiles, ntn, tpx;     // persistent: 256-row tiles, tiles per row block, tiles per XCD run
  int wgs;                 // persistent: workgroups (== gx)
  long long counter_bytes; // what the fused entry asks of the caller
  bool reads_cus;          // past the shape, K and m == 0 tests: what follows read in.cus
};

constexpr long long kGemm2G = 1ll << 31;
// What kernels.linear_fn (forward, dgrad and wgrad of one shape) is routed up to: x, dy and dx
// of m rows each under this many bytes, m * max(n, k) * 2 < kLinearFnMaxBytes.  The plans
// accept more (the persistent form takes x past 2 GB); nothing past this is tested.
constexpr long long kLinearFnMaxBytes = kGemm2G;

// The plan input of vm_linear_fwd_form, vm_linear_dgrad (`dgrad`: the caller passes dy / wT /
// dx with n and k swapped) and vm_linear_fits: the entries and the query build it here, so
// they cannot disagree.  `cus` 0 until a caller has looked it up.
inline GemmPlanIn gemm_linear_in(int m, int n, int k, long long ldx, long long ldw,
                                 long long ldo, bool has_bias, bool bf16, int form, bool x_al,
                                 bool w_al, bool o_al, bool dgrad = false) {
  GemmPlanIn in{};
  in.m = m; in.n = n; in.k = k; in.ldx = ldx; in.ldw = ldw; in.ldo = ldo;
  in.has_bias = has_bias; in.bf16 = bf16; in.form = form;
  in.x_al = x_al; in.w_al = w_al; in.o_al = o_al;
  in.dgrad = dgrad;
  return in;
}
// ... and of vm_linear_add_norm_fwd and vm_linear_add_norm_fits.
inline GemmPlanIn gemm_add_norm_in(int m, int n, int k, long long ldx, long long ldw,
                                   long long ldo, long long ldr, long long ldh, bool x_al,
                                   bool w_al, bool o_al, bool r_al, bool nw_al, bool hn_al,
                                   long long counter_bytes) {
  GemmPlanIn in = gemm_linear_in(m, n, k, ldx, ldw, ldo, false, true, 0, x_al, w_al, o_al);
  in.ldr = ldr; in.ldh = ldh;
  in.r_al = r_al; in.nw_al = nw_al; in.hn_al = hn_al;
  in.counter_bytes = counter_bytes;
  return in;
}

// The persistent tile width of a shape, 0 when it has none: wide n on 256 columns, else 192
// where it divides n, else 256; each tile's buffer ranges (256 rows of x / out, bn rows of w)
// under 2^31 bytes.
inline int gemm_tile_bn(int n, int k, long long ldx, long long ldw, long long ldo,
                        bool dgrad = false) {
  if (!(dgrad ? gemm_dgrad_k_ok(k) : gemm_k_ok(k))) return 0;
  const int bn = (n >= 1024 && n % kTileBNWide == 0) ? kTileBNWide
                 : n % kTileBNNarrow == 0            ? kTileBNNarrow
                 : n % kTileBNWide == 0              ? kTileBNWide : 0;
  if (!bn) return 0;
  if (kTileBM * ldx * 2 >= kGemm2G || kTileBM * ldo * 2 >= kGemm2G || bn * ldw * 2 >= kGemm2G)
    return 0;
  return bn;
}
inline long long gemm_tile_count(int m, int n, int bn) {
  return gemm_ceil_div(m, kTileBM) * (n / bn);
}
constexpr int gemm_tile_wgs(int cus) { return cus / 8 * 8; }  // whole XCD runs
// THE persistent test of form 0, for vm_linear_fwd and the fused entry alike (the fused
// entry's bits equal "what vm_linear_fwd would pick" because both call this).
inline bool gemm_tile_fills(int m, int n, int bn, int cus) {
  const int wgs = gemm_tile_wgs(cus);
  return bn && wgs >= 8 &&
         2 * gemm_tile_count(m, n, bn) >= static_cast<long long>(kTileMinPerCU2) * wgs;
}
constexpr bool gemm_tile_norm_ok(int n, int k, int bn) {
  if (bn != kTileBNNarrow) return false;
#define VM_GEMM_NORM_IS(NV, KV) if (n == NV && k == KV) return true;
  VM_GEMM_TILE_NORM_LIST(VM_GEMM_NORM_IS)
#undef VM_GEMM_NORM_IS
  return false;
}

namespace gemm_detail {
inline GemmPlan refuse(GemmPlan pl, GemmWhy why) {
  pl.form = GemmForm::kNone;
  pl.why = why;
  return pl;
}
inline void set_tile(GemmPlan& pl, const GemmPlanIn& in, GemmForm form, int bn) {
  pl.form = form;
  pl.bn = bn;
  pl.ntn = in.n / bn;
  pl.tiles = static_cast<int>(gemm_tile_count(in.m, in.n, bn));
  pl.tpx = (pl.tiles + 7) / 8;
  if (form == GemmForm::kTileNorm) {  // whole row blocks per XCD run
    pl.tpx = (pl.tpx + pl.ntn - 1) / pl.ntn * pl.ntn;
    pl.NC = (in.n + 255) / 256;
  }
  pl.wgs = gemm_tile_wgs(in.cus);
  pl.gx = static_cast<unsigned>(pl.wgs);
  pl.gy = 1;
  pl.block = kTileThreads;
  pl.lds = tile_lds(bn);
}
inline void set_dma(GemmPlan& pl, const GemmPlanIn& in, GemmForm form, const DmaTile& t,
                    size_t lds) {
  pl.form = form;
  pl.bn = t.bn;
  pl.gx = static_cast<unsigned>(gemm_ceil_div(in.m, t.bm));
  pl.gy = static_cast<unsigned>(gemm_ceil_div(in.n, t.bn));
  pl.block = t.threads();
  pl.lds = lds;
}
}  // namespace gemm_detail

// vm_linear_fwd_form and vm_linear_dgrad (in.dgrad).  The order of the tests is the order of
// the refusals a caller sees.
inline GemmPlan plan_linear(const GemmPlanIn& in) {
  using namespace gemm_detail;
  GemmPlan pl{};
  pl.form = GemmForm::kNone;
  pl.why = GemmWhy::kOk;
  if (in.form < 0 || in.form > 2) return refuse(pl, GemmWhy::kFormArg);
  if (!in.bf16 || in.m < 0 || in.n < 1 || in.k < kGemmBK || in.n % 8 || in.k % kGemmBK ||
      in.ldx < in.k || in.ldw < in.k || in.ldo < in.n || in.ldx % 8 || in.ldw % 8 ||
      in.ldo % 8 || !in.x_al || !in.w_al || !in.o_al || in.n * in.ldw * 2 >= kGemm2G)
    return refuse(pl, GemmWhy::kShape);
  if (!(in.dgrad ? gemm_dgrad_k_ok(in.k) : gemm_k_ok(in.k))) return refuse(pl, GemmWhy::kK);
  pl.NK = in.k / kGemmBK;
  if (in.m == 0) {
    pl.form = GemmForm::kEmpty;
    return pl;
  }
  pl.reads_cus = true;
  const int bn = in.has_bias ? 0 : gemm_tile_bn(in.n, in.k, in.ldx, in.ldw, in.ldo, in.dgrad);
  if (in.form == 2 && !bn) return refuse(pl, GemmWhy::kTileShape);
  if (in.form == 2 && gemm_tile_wgs(in.cus) < 8) return refuse(pl, GemmWhy::kTileCus);
  if (in.form == 2 || (in.form == 0 && gemm_tile_fills(in.m, in.n, bn, in.cus))) {
    set_tile(pl, in, bn == kTileBNWide ? GemmForm::kTile256 : GemmForm::kTile192, bn);
    return pl;
  }
  if (in.m * in.ldx * 2 >= kGemm2G) return refuse(pl, GemmWhy::kXPast2GB);
  if (in.n >= kDmaWideMinN) set_dma(pl, in, GemmForm::kDma128x128, kDmaWide, kDmaWide.lds());
  else set_dma(pl, in, GemmForm::kDma128x64, kDmaNarrow, kDmaNarrow.lds());
  return pl;
}

// vm_linear_add_norm_fwd (no bias, bf16, form 0).
inline GemmPlan plan_linear_add_norm(const GemmPlanIn& in) {
  using namespace gemm_detail;
  GemmPlan pl{};
  pl.form = GemmForm::kNone;
  pl.why = GemmWhy::kOk;
  pl.counter_bytes = gemm_counter_bytes(in.m);
  if (in.m < 0 || in.n < 4 || in.n > kNormMaxN || in.n % 8 || in.k < kGemmBK ||
      in.k % kGemmBK || in.ldx < in.k || in.ldw < in.k || in.ldo < in.n || in.ldr < in.n ||
      in.ldh < in.n || in.ldx % 8 || in.ldw % 8 || in.ldo % 8 || in.ldr % 4 || in.ldh % 4 ||
      !in.x_al || !in.w_al || !in.o_al || !in.r_al || !in.nw_al || !in.hn_al ||
      in.n * in.ldw * 2 >= kGemm2G || in.counter_bytes < pl.counter_bytes)
    return refuse(pl, GemmWhy::kNormShape);
  if (!gemm_k_ok(in.k)) return refuse(pl, GemmWhy::kNormK);
  pl.NK = in.k / kGemmBK;
  if (in.m == 0) {
    pl.form = GemmForm::kEmpty;
    return pl;
  }
  pl.reads_cus = true;
  // One launch when the whole grid is co-resident at one workgroup per CU: a consumer's poll
  // then never waits on an undispatched producer.  (Its x and h go through one 31-bit buffer
  // each; rows past that take the forms below, which have their own limits.)
  const DmaTile& t = kDmaNormTile;
  const long long nwg = gemm_ceil_div(in.m, t.bm) * gemm_ceil_div(in.n, t.bn);
  if (in.cus > 0 && nwg <= in.cus && in.m * in.ldx * 2 < kGemm2G && in.m * in.ldo * 2 < kGemm2G) {
    set_dma(pl, in, GemmForm::kDmaNorm, t, kDmaNormLds);
    return pl;
  }
  // chip-filling row counts: the persistent kernel's NORM form, where vm_linear_fwd would
  // pick the persistent kernel
  const int bn = gemm_tile_bn(in.n, in.k, in.ldx, in.ldw, in.ldo);
  if (gemm_tile_norm_ok(in.n, in.k, bn) && gemm_tile_fills(in.m, in.n, bn, in.cus)) {
    set_tile(pl, in, GemmForm::kTileNorm, bn);
    return pl;
  }
  // otherwise the two launches it replaces (the same kernels: bit-identical either way)
  if (in.ldo != in.n || in.ldr != in.n || in.ldh != in.n) return refuse(pl, GemmWhy::kNormStrides);
  pl.form = GemmForm::kTwoLaunch;
  return pl;
}

// The fits queries: whether the plan takes the call, on `in.cus` CUs.
inline bool linear_fits(const GemmPlanIn& in) { return plan_linear(in).form != GemmForm::kNone; }
inline bool linear_add_norm_fits(const GemmPlanIn& in) {
  return plan_linear_add_norm(in).form != GemmForm::kNone;
}

}  // namespace vm

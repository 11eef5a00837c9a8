// Host-side plan of the projection GEMM's weight gradient (vm_gemm_wgrad.hip):
//   dw[n, k] = sum over m of dy[m, n] * x[m, k]
// which output tile and which slice of m every workgroup owns, where its fp32 partial tile
// lies in the caller's workspace, the refusals and both launch geometries.  Plain C++17, no
// HIP header: the size query, the entry's checks and both launches read one WgradPlan, the
// kernels take the tile and stage constants below, and tests/host/gemm_wgrad_plan_check.cpp
// walks plan_linear_wgrad() over a grid of shapes on the host.  The plan takes (m, n, k) and
// the strides only, never a CU count, so the order of every sum is the same on every device.
//
// A workgroup owns one kWgTileN x kWgTileK output tile and one slice of m: rows
// [s slice_rows, min(m, (s + 1) slice_rows)).  It walks the slice in stages of kWgStageRows
// rows and stores its partial tile to part[s][n][k] (fp32, row stride k).  The reduce kernel
// adds the slices of every element in slice order and rounds once.
//
// Slices: kWgMinSliceRows rows each until there would be more than max_slices of them, then
// max_slices slices of equal length (a multiple of kWgStageRows), with
//   max_slices = max(kWgMinSlices, floor(kWgTargetWgs / tiles)):
// tiles x slices stays within kWgTargetWgs workgroups (one round of two per CU on 256 CUs)
// wherever tiles <= kWgTargetWgs / kWgMinSlices.
// Workspace: 4 n k min(max_slices, ceil(m / kWgMinSliceRows)) bytes, which never shrinks as m
// grows (the slices in use may be one fewer just past a step of slice_rows).  Upper bound for
// any m, from tiles >= n k / (kWgTileN kWgTileK):
//   workspace_bytes <= 4 (kWgMinSlices n k + kWgTargetWgs kWgTileN kWgTileK)
//                    = 16 n k + 32 MiB
// VideoMamba-M in_proj (n 2304, k 576; 90 tiles, 5 slices): 25.3 MiB at B = 8 and B = 32;
// out_proj (n 576, k 1152; 45 tiles, 11 slices): 27.8 MiB.
#pragma once

#include <cstddef>

#include "vm_gemm_plan.h"

namespace vm {

constexpr int kWgTileN = 128;       // output rows per tile (columns of dy)
constexpr int kWgTileK = 128;       // output columns per tile (columns of x)
constexpr int kWgStageRows = 32;    // rows of m per LDS stage: one 16x16x32 MFMA step
constexpr int kWgStages = 4;        // stage buffers (three stages in flight)
constexpr int kWgRowBytes = 256;    // one staged row of either operand: 128 bf16
constexpr unsigned kWgThreads = 256;  // 4 waves, 2 (n) x 2 (k), 64 x 64 outputs each
constexpr size_t kWgLdsBytes =
    static_cast<size_t>(kWgStages) * kWgStageRows * 2 * kWgRowBytes;  // 64 KiB
constexpr int kWgMinSliceRows = 256;
constexpr int kWgMinSlices = 4;
constexpr int kWgTargetWgs = 512;   // two workgroups per CU of a 256-CU chip
constexpr unsigned kWgReduceThreads = 256;  // one thread per 4 columns of dw
constexpr long long kWg2G = 1ll << 31;

constexpr long long wgrad_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
constexpr long long wgrad_ws_bound(int n, int k) {
  return 4ll * (static_cast<long long>(kWgMinSlices) * n * k +
                static_cast<long long>(kWgTargetWgs) * kWgTileN * kWgTileK);
}

enum class WgradWhy {
  kOk,
  kDtype,      // operands other than bf16, dw other than bf16 / fp32
  kShape,      // m < 0, n or k out of range, n % 8, k % 64
  kStrides,    // a leading dimension below the width or no multiple of 8
  kAlign,      // a pointer off 16 bytes
  kPast2GB,    // dy or x past what one 31-bit buffer addresses
  kWorkspace,  // workspace below the query (or missing)
};

struct WgradPlanIn {
  int m, n, k;
  long long lddy, ldx, lddw;   // row strides, in elements
  bool bf16;                   // dtype == VM_DTYPE_BF16 (dy and x)
  bool dw_dtype_ok;            // dw_dtype is VM_DTYPE_BF16 or VM_DTYPE_F32
  bool dy_al, x_al, dw_al, ws_al;  // 16-byte alignment (ws_al: true for a null workspace)
  long long workspace_bytes;   // what the caller gave
};

struct WgradPlan {
  WgradWhy why;
  bool empty;                  // m == 0: only the reduce kernel runs and writes zeros
  int tiles_n, tiles_k;        // output tiles
  long long slice_rows;        // rows of m per slice, a multiple of kWgStageRows
  int slices;                  // slices in use: ceil(m / slice_rows)
  int max_slices;
  unsigned gx, gy, gz, block;  // partial kernel: (tiles_k, tiles_n, slices); gz == 0: no launch
  size_t lds;
  unsigned rgx, rblock;        // reduce kernel
  long long workspace_bytes;   // what the query answers
  constexpr long long row_begin(int s) const { return s * slice_rows; }
  constexpr long long row_end(int s, long long m) const {
    return (s + 1) * slice_rows < m ? (s + 1) * slice_rows : m;
  }
  // float offset of part[s][0][0]
  constexpr size_t part_offset(int s, int n, int k) const {
    return static_cast<size_t>(s) * n * k;
  }
};

// The geometry of a shape (what vm_linear_wgrad_workspace_bytes reads): no refusals.
inline WgradPlan plan_linear_wgrad_shape(int m, int n, int k) {
  WgradPlan pl{};
  pl.why = WgradWhy::kOk;
  if (m < 0) m = 0;
  if (n < 0) n = 0;
  if (k < 0) k = 0;
  pl.tiles_n = static_cast<int>(wgrad_ceil_div(n, kWgTileN));
  pl.tiles_k = static_cast<int>(wgrad_ceil_div(k, kWgTileK));
  const long long tiles = static_cast<long long>(pl.tiles_n) * pl.tiles_k;
  long long ms = tiles > 0 ? kWgTargetWgs / tiles : kWgMinSlices;
  if (ms < kWgMinSlices) ms = kWgMinSlices;
  pl.max_slices = static_cast<int>(ms);
  long long rows = wgrad_ceil_div(wgrad_ceil_div(m, ms), kWgStageRows) * kWgStageRows;
  if (rows < kWgMinSliceRows) rows = kWgMinSliceRows;
  pl.slice_rows = rows;
  pl.slices = static_cast<int>(wgrad_ceil_div(m, rows));
  pl.empty = m == 0 || tiles == 0;
  long long ws_slices = wgrad_ceil_div(m, kWgMinSliceRows);
  if (ws_slices > ms) ws_slices = ms;
  pl.workspace_bytes = 4ll * n * k * ws_slices;
  pl.gx = static_cast<unsigned>(pl.tiles_k);
  pl.gy = static_cast<unsigned>(pl.tiles_n);
  pl.gz = pl.empty ? 0u : static_cast<unsigned>(pl.slices);
  pl.block = kWgThreads;
  pl.lds = kWgLdsBytes;
  pl.rblock = kWgReduceThreads;
  pl.rgx = static_cast<unsigned>(
      wgrad_ceil_div(static_cast<long long>(n) * (k / 4), kWgReduceThreads));
  return pl;
}

// vm_linear_wgrad.  The order of the tests is the order of the refusals a caller sees.
inline WgradPlan plan_linear_wgrad(const WgradPlanIn& in) {
  WgradPlan pl = plan_linear_wgrad_shape(in.m, in.n, in.k);
  auto refuse = [&](WgradWhy why) {
    pl.why = why;
    pl.gz = 0;
    pl.rgx = 0;
    return pl;
  };
  if (!in.bf16 || !in.dw_dtype_ok) return refuse(WgradWhy::kDtype);
  if (in.m < 0 || in.n < 8 || in.k < 64 || in.n % 8 || in.k % 64 ||
      static_cast<long long>(in.n) * in.k >= kWg2G / 4)
    return refuse(WgradWhy::kShape);
  if (in.lddy < in.n || in.ldx < in.k || in.lddw < in.k || in.lddy % 8 || in.ldx % 8 ||
      in.lddw % 8)
    return refuse(WgradWhy::kStrides);
  if (!in.dy_al || !in.x_al || !in.dw_al || !in.ws_al) return refuse(WgradWhy::kAlign);
  if (in.m * in.lddy * 2 >= kWg2G || in.m * in.ldx * 2 >= kWg2G)
    return refuse(WgradWhy::kPast2GB);
  if (in.workspace_bytes < pl.workspace_bytes) return refuse(WgradWhy::kWorkspace);
  return pl;
}

// vm_linear_fn_fits: forward, dgrad and wgrad all take row-contiguous, 16-byte aligned bf16
// operands of x (m, k), w (n, k), on `cus` CUs: plan_linear on x, plan_linear with dgrad on
// dy (m, n) / wT (k, n), plan_linear_wgrad offered its own query's workspace, under
// kLinearFnMaxBytes.
inline bool linear_fn_fits(int m, int n, int k, int cus) {
  if (m <= 0 || n <= 0 || k <= 0 ||
      static_cast<long long>(m) * (n > k ? n : k) * 2 >= kLinearFnMaxBytes)
    return false;
  GemmPlanIn fwd = gemm_linear_in(m, n, k, k, k, n, false, true, 0, true, true, true);
  GemmPlanIn dgrad = gemm_linear_in(m, k, n, n, n, k, false, true, 0, true, true, true, true);
  fwd.cus = dgrad.cus = cus;
  WgradPlanIn wg{};
  wg.m = m; wg.n = n; wg.k = k; wg.lddy = n; wg.ldx = k; wg.lddw = k;
  wg.bf16 = wg.dw_dtype_ok = wg.dy_al = wg.x_al = wg.dw_al = wg.ws_al = true;
  wg.workspace_bytes = plan_linear_wgrad_shape(m, n, k).workspace_bytes;
  return linear_fits(fwd) && linear_fits(dgrad) && plan_linear_wgrad(wg).why == WgradWhy::kOk;
}

}  // namespace vm

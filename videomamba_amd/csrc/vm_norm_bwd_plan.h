// Host-side plan of the add + norm backward (vm_norm_bwd.hip): which rows every workgroup
// owns, where its dweight / dbias column partials lie in the caller's workspace and the
// ranges the second kernel adds them in.  Plain C++17, no HIP header: the size query, the
// entry's workspace check and both launches read one NormBwdPlan, and
// tests/host/norm_bwd_plan_check.cpp walks plan_norm_bwd() over a grid of shapes on the host.
// It takes (rows, cols) only, so the order of every sum is the same on every device.
//
// A workgroup is one wave.  It owns rows [wg rows_per_wg, (wg + 1) rows_per_wg), holds one
// row at a time in registers and adds its column partials in row order.
// Workspace, in floats from the workspace base (cpad = round_up(cols, 64)):
//   part [nwg][2][cpad]     [0]: sum over the workgroup's rows of dy * xhat, [1]: of dy
// In bytes 8 nwg cpad with nwg <= min(kNbMaxWgs, ceil(rows / kNbMinRows)): at most
// 8 cpad min(2048, rows / 4 + 1), 32 MiB at cols = 2048.
// The reduce kernel gives one thread (column, which, range r): it adds workgroups
// [r per_range, (r + 1) per_range) in workgroup order, then the kNbRanges range sums are
// added in range order.
#pragma once

#include <cstddef>

namespace vm {

constexpr int kNbMaxCols = 2048;
constexpr int kNbMaxWgs = 2048;  // workgroups at most: two waves per SIMD of a 256-CU chip
constexpr int kNbMinRows = 4;    // rows per workgroup at least
constexpr int kNbRanges = 16;    // contiguous workgroup ranges of the reduce kernel

struct NormBwdPlan {
  long long rows_per_wg;
  int nwg;    // workgroups, every one with at least one row (0 without rows)
  int cpad;   // columns rounded up to 64
  int per_range;  // workgroups per reduce range (the last ranges may be short or empty)
  size_t ws_bytes;
  constexpr long long row_begin(int wg) const { return wg * rows_per_wg; }
  constexpr long long row_end(int wg, long long rows) const {
    return (wg + 1) * rows_per_wg < rows ? (wg + 1) * rows_per_wg : rows;
  }
  // float offset of column 0 of (workgroup, which)
  constexpr size_t part_offset(int wg, int which) const {
    return (static_cast<size_t>(wg) * 2 + which) * cpad;
  }
  constexpr int range_begin(int r) const { return r * per_range < nwg ? r * per_range : nwg; }
  constexpr int range_end(int r) const { return range_begin(r + 1); }
};

inline NormBwdPlan plan_norm_bwd(long long rows, int cols) {
  NormBwdPlan pl{};
  if (rows < 0) rows = 0;
  if (cols < 0) cols = 0;
  long long rpw = (rows + kNbMaxWgs - 1) / kNbMaxWgs;
  if (rpw < kNbMinRows) rpw = kNbMinRows;
  pl.rows_per_wg = rpw;
  pl.nwg = cols > 0 ? static_cast<int>((rows + rpw - 1) / rpw) : 0;
  pl.cpad = (cols + 63) / 64 * 64;
  pl.per_range = (pl.nwg + kNbRanges - 1) / kNbRanges;
  pl.ws_bytes = static_cast<size_t>(pl.nwg) * 2 * pl.cpad * sizeof(float);
  return pl;
}

}  // namespace vm

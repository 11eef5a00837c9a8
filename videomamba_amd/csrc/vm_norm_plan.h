// Host-side plan of the norm forward (vm_norm.hip): which kernel instance an add + norm, a
// norm + pool or a pool finish call launches, on which grid, and where the pooling sums lie in
// the caller's workspace.  Plain C++17, no HIP header: the size query, the entries' checks and
// the launches read one plan each, and tests/host/norm_fwd_plan_check.cpp walks the three
// planners over grids of shapes on the host (tests/host/norm_fwd_instance_of.cpp prints the
// planned instance of a case for the tests' own restatement of these rules).
//
// Add + norm (plan_add_norm).  A workgroup is four waves, one row each: grid ceil(rows / 4).
//   kFast    add_rms_bf16_kernel<cpl, res, ro, write_through>: the vector form's conditions
//            and RMSNorm, no bias, bf16 x / out, fp32 (or no) residual and residual_out,
//            cols <= kNormFastMaxCols; cpl = ceil(cols / 256) in {1, 2, 3, 4}.  The stores
//            write through (kSmallStoreWT) iff res && ro && rows <= kSmallStoreRows.
//   kVec     add_norm_vec_kernel<cpl>: cols % 4 == 0 and every pointer given on 16 bytes;
//            cpl the smallest of {1, 2, 4, 8} with 256 cpl >= cols.
//   kScalar  add_norm_kernel<vpl>: everything else; vpl the smallest of {4, 8, 16, 32} with
//            64 vpl >= cols (the plan's cpl field holds it).
// Refusals in the order a caller sees them: a null x / weight / out, then shape / dtype
// (rows < 0, cols outside [1, kNormMaxCols], a dtype code that is none of the two).
//
// Norm + pool (plan_norm_pool).  Grid (max(slices, ceil(head / kPoolRB)), groups + 1, batch):
// y == 0 is the head, y == g + 1 group g, x the kPoolRB-row slice; LDS 4 rows of cols floats.
//   kFast    norm_pool_rows_bf16_kernel<cpl>: bf16 x / out, fp32 (or no) residual,
//            cols <= kNormFastMaxCols and (rows + 1) cols 4 < kNorm2G (one 31-bit buffer
//            offset reaches every row of a batch row); cpl = ceil(cols / 256).
//   kGeneric norm_pool_rows_kernel<cpl>: cpl the smallest of {1, 2, 4, 8}.
// Workspace, in floats from its base: part[batch][groups][slices][cols], back to back, with
//   slices = pool_slices(max_group_rows) = max(1, ceil(max_group_rows / kPoolRB)),
// the one slice count of the query, the forward's check, the launch and the finish.  Groups
// without rows (max_group_rows == 0: a head-only call) still own one slice each, which the
// forward writes zeros to.
// Refusals in order: null pointer, shape / dtype / strides / tiling, alignment, workspace.
//
// Pool finish (plan_pool_finish).  Grid (prow, batch) of 1024 threads, prow the pooled rows
// per batch row: 1 (cls), groups or 1 (avg, cls+avg: with / without keep_temporal), one more
// for cls_cat_avg.  Refusals in order: null pointer, mode / shape / dtype.
#pragma once

namespace vm {

constexpr int kNormMaxCols = 2048;        // columns of any norm forward entry
constexpr int kNormFastMaxCols = 1024;    // columns of the two bf16 buffer-load kernels
constexpr long long kNorm2G = 1ll << 31;  // bytes one buffer offset addresses
constexpr int kPoolRB = 16;               // rows of one pooling slice (one workgroup)
constexpr unsigned kNormThreads = 256;    // four waves
constexpr unsigned kPoolFinishThreads = 1024;
// add + RMSNorm calls of up to this many rows (the streaming chunks) store with kSmallStoreWT
constexpr long long kSmallStoreRows = 32768;
// VM_DTYPE_F32 / VM_DTYPE_BF16 of videomamba_hip.h (vm_norm.hip asserts the values)
constexpr int kNormF32 = 0, kNormBf16 = 1;

constexpr bool norm_dtype_ok(int d) { return d == kNormF32 || d == kNormBf16; }
constexpr long long norm_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
// the smallest of {lo, 2 lo, 4 lo, 8 lo} that is >= need (8 lo past that)
constexpr int norm_step_up(int need, int lo) {
  return need <= lo ? lo : need <= 2 * lo ? 2 * lo : need <= 4 * lo ? 4 * lo : 8 * lo;
}
constexpr int pool_slices(int max_group_rows) {
  const int n = static_cast<int>(norm_ceil_div(max_group_rows, kPoolRB));
  return n > 1 ? n : 1;
}

enum class NormWhy {
  kOk,
  kNull,       // a required pointer is null
  kShape,      // shape, dtype, strides or group tiling
  kAlign,      // a pointer off 16 bytes (norm + pool)
  kWorkspace,  // a workspace below the query
};
enum class NormFamily { kFast, kVec, kScalar, kGeneric };

// ------------------------------------------------------------------------ add + norm
struct AddNormPlanIn {
  long long rows;
  int cols;
  bool is_rms;
  bool has_x, has_weight, has_out;        // the required pointers
  bool has_bias, has_res, has_ro;
  int x_dtype, res_dtype, out_dtype, ro_dtype;  // as the entry receives them
  bool x_al, res_al, w_al, out_al, ro_al;  // 16-byte alignment (read only where present)
};

struct AddNormPlan {
  NormWhy why;
  bool empty;          // rows == 0: VM_OK without a launch
  NormFamily family;
  int cpl;             // chunks per lane (kFast, kVec) or values per lane (kScalar)
  bool res, ro;        // kFast: the RES / RO template arguments
  bool write_through;  // kFast: stores with kSmallStoreWT
  unsigned grid, block;
};

inline AddNormPlan plan_add_norm(const AddNormPlanIn& in) {
  AddNormPlan pl{};
  pl.why = NormWhy::kOk;
  if (!in.has_x || !in.has_weight || !in.has_out) {
    pl.why = NormWhy::kNull;
    return pl;
  }
  if (in.rows < 0 || in.cols < 1 || in.cols > kNormMaxCols || !norm_dtype_ok(in.x_dtype) ||
      !norm_dtype_ok(in.out_dtype) || (in.has_res && !norm_dtype_ok(in.res_dtype)) ||
      (in.has_ro && !norm_dtype_ok(in.ro_dtype))) {
    pl.why = NormWhy::kShape;
    return pl;
  }
  pl.empty = in.rows == 0;
  pl.grid = static_cast<unsigned>(norm_ceil_div(in.rows, 4));
  pl.block = kNormThreads;
  const bool vec = in.cols % 4 == 0 && in.x_al && in.out_al && in.w_al &&
                   (!in.has_res || in.res_al) && (!in.has_ro || in.ro_al);
  const int chunks = static_cast<int>(norm_ceil_div(in.cols, 256));
  if (vec && in.is_rms && !in.has_bias && in.x_dtype == kNormBf16 && in.out_dtype == kNormBf16 &&
      (!in.has_res || in.res_dtype == kNormF32) && (!in.has_ro || in.ro_dtype == kNormF32) &&
      in.cols <= kNormFastMaxCols) {
    pl.family = NormFamily::kFast;
    pl.cpl = chunks;
    pl.res = in.has_res;
    pl.ro = in.has_ro;
    pl.write_through = pl.res && pl.ro && in.rows <= kSmallStoreRows;
  } else if (vec) {
    pl.family = NormFamily::kVec;
    pl.cpl = norm_step_up(chunks, 1);
  } else {
    pl.family = NormFamily::kScalar;
    pl.cpl = norm_step_up(static_cast<int>(norm_ceil_div(in.cols, 64)), 4);
  }
  return pl;
}

// ------------------------------------------------------------------------ norm + pool
struct NormPoolPlanIn {
  int batch, rows, cols, head, groups, group_rows, max_group_rows, rev_frame;
  long long in_bstride, out_bstride;      // elements between batch rows
  bool has_x, has_weight, has_out;        // the required pointers
  bool has_res, has_bounds, has_ws;
  int x_dtype, res_dtype, out_dtype;
  bool x_al, res_al, w_al, out_al;
  long long workspace_bytes;              // what the caller gave
};

struct NormPoolPlan {
  NormWhy why;
  bool empty;          // batch == 0 or rows == 0: VM_OK without a launch
  NormFamily family;   // kFast or kGeneric
  int cpl;
  int groups, slices;
  unsigned gx, gy, gz, block;
  unsigned lds;        // bytes
  long long workspace_bytes;  // what the query answers
  // float offset of column 0 of part[b][g][s]
  constexpr long long part_offset(int b, int g, int s, int cols) const {
    return ((static_cast<long long>(b) * groups + g) * slices + s) * cols;
  }
};

// The layout of a shape (what vm_norm_pool_workspace_bytes reads): no refusals.
inline NormPoolPlan plan_norm_pool_shape(int batch, int groups, int max_group_rows, int cols) {
  NormPoolPlan pl{};
  pl.why = NormWhy::kOk;
  pl.groups = groups;
  pl.slices = pool_slices(max_group_rows);
  pl.workspace_bytes = 4ll * batch * groups * pl.slices * cols;
  return pl;
}

inline NormPoolPlan plan_norm_pool(const NormPoolPlanIn& in) {
  NormPoolPlan pl = plan_norm_pool_shape(in.batch, in.groups, in.max_group_rows, in.cols);
  auto refuse = [&](NormWhy why) {
    pl.why = why;
    return pl;
  };
  if (!in.has_x || !in.has_weight || !in.has_out) return refuse(NormWhy::kNull);
  const long long used = static_cast<long long>(in.rows) * in.cols;
  if (in.batch < 0 || in.rows < 0 || in.cols < 4 || in.cols > kNormMaxCols || in.cols % 4 ||
      in.head < 0 || in.head > in.rows || in.groups < 1 || in.max_group_rows < 0 ||
      in.in_bstride < used || in.in_bstride % 4 || in.out_bstride < used || in.out_bstride % 4 ||
      in.rev_frame < 0 || (in.rev_frame > 0 && (in.rows - in.head) % in.rev_frame) ||
      !norm_dtype_ok(in.x_dtype) || !norm_dtype_ok(in.out_dtype) ||
      (in.has_res && !norm_dtype_ok(in.res_dtype)) ||
      (!in.has_bounds &&
       in.head + static_cast<long long>(in.groups) * in.group_rows != in.rows) ||
      (!in.has_bounds && in.group_rows != in.max_group_rows))
    return refuse(NormWhy::kShape);
  if (!in.x_al || !in.out_al || !in.w_al || (in.has_res && !in.res_al))
    return refuse(NormWhy::kAlign);
  if (in.has_ws && in.workspace_bytes < pl.workspace_bytes) return refuse(NormWhy::kWorkspace);
  pl.empty = in.batch == 0 || in.rows == 0;
  // x: the kPoolRB-row slices of a group, or of the head rows where those are more
  const int head_slices = static_cast<int>(norm_ceil_div(in.head, kPoolRB));
  pl.gx = static_cast<unsigned>(pl.slices > head_slices ? pl.slices : head_slices);
  pl.gy = static_cast<unsigned>(in.groups) + 1;
  pl.gz = static_cast<unsigned>(in.batch);
  pl.block = kNormThreads;
  pl.lds = 4u * static_cast<unsigned>(in.cols) * 4u;
  const bool fast = in.x_dtype == kNormBf16 && in.out_dtype == kNormBf16 &&
                    (!in.has_res || in.res_dtype == kNormF32) &&
                    in.cols <= kNormFastMaxCols && (in.rows + 1ll) * in.cols * 4 < kNorm2G;
  const int chunks = static_cast<int>(norm_ceil_div(in.cols, 256));
  pl.family = fast ? NormFamily::kFast : NormFamily::kGeneric;
  pl.cpl = fast ? chunks : norm_step_up(chunks, 1);
  return pl;
}

// ------------------------------------------------------------------------ pool finish
enum PoolMode { kPoolAvg = 0, kPoolClsAvg = 1, kPoolClsCatAvg = 2, kPoolCls = 3 };

struct PoolFinishPlanIn {
  int batch, groups, max_group_rows, cols, mode, keep_temporal;
  bool has_ws, has_cls, has_xpool;
  int cls_dtype, xp_dtype;
};

struct PoolFinishPlan {
  NormWhy why;
  bool empty;        // batch == 0: VM_OK without a launch
  int slices;
  int prow;          // pooled rows per batch row
  unsigned gx, gy, block;
};

inline PoolFinishPlan plan_pool_finish(const PoolFinishPlanIn& in) {
  PoolFinishPlan pl{};
  pl.why = NormWhy::kOk;
  const bool needs_cls = in.mode == kPoolClsAvg || in.mode == kPoolClsCatAvg || in.mode == kPoolCls;
  const bool needs_avg = in.mode != kPoolCls;
  if (!in.has_xpool || (needs_cls && !in.has_cls) || (needs_avg && !in.has_ws)) {
    pl.why = NormWhy::kNull;
    return pl;
  }
  if (in.batch < 0 || in.groups < 1 || in.mode < kPoolAvg || in.mode > kPoolCls || in.cols < 4 ||
      in.cols > kNormMaxCols || in.cols % 4 || in.max_group_rows < 1 ||
      !norm_dtype_ok(in.xp_dtype) || (in.has_cls && !norm_dtype_ok(in.cls_dtype))) {
    pl.why = NormWhy::kShape;
    return pl;
  }
  pl.empty = in.batch == 0;
  pl.slices = pool_slices(in.max_group_rows);
  const int navg = in.keep_temporal ? in.groups : 1;
  pl.prow = in.mode == kPoolCls ? 1 : (in.mode == kPoolClsCatAvg ? 1 + navg : navg);
  pl.gx = static_cast<unsigned>(pl.prow);
  pl.gy = static_cast<unsigned>(in.batch);
  pl.block = kPoolFinishThreads;
  return pl;
}

}  // namespace vm

// Backward of the fused residual add + RMSNorm / LayerNorm (vm_add_norm_fwd).  With s the
// pre-norm sum the forward wrote as residual_out, statistics recomputed from it in the
// forward's order (its own bits when s is fp32), xhat = (s - mean) rstd and g = dy w:
//   RMSNorm:   ds = rstd (g - xhat mean(g xhat))
//   LayerNorm: ds = rstd (g - mean(g) - xhat mean(g xhat))
//   ds += dres_out;  dx = dresidual = ds, each rounded once to its own dtype
//   dweight = sum_rows dy xhat,  dbias = sum_rows dy
// all in fp32.
//
// A workgroup is one wave; it owns a contiguous range of rows (vm_norm_bwd_plan.h), holds one
// row in registers as the forward does — lane l the 4-column chunks l*4 + 256 j, or columns
// l + 64 j without the vector path — loads the next row before it works on the current one,
// and adds its dweight / dbias column partials in row order.  norm_bwd_reduce_kernel adds the
// workgroups' partials in a fixed order.  No atomics.
//
// Bounds: a chunk past `cols` re-reads chunk 0 of its row and is used as 0, so no load sits
// under a lane-dependent branch; such a chunk stores nothing.

#include "vm_common.h"
#include "vm_norm_bwd_plan.h"

namespace vm {

struct NormBwdParams {
  const void* s; const float* w; const void* dy; const void* dres;
  void* dx; void* dr; float* dw; float* db;
  long long rows; int cols; float eps;
  int is_rms, s_dtype, dy_dtype, dx_dtype, dr_dtype;
};

__device__ __forceinline__ float nb_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
struct alignas(sizeof(T) * 4) Quad {
  T v[4];
};

__device__ __forceinline__ void nb_store4(void* p, long long i, int dtype, const float (&v)[4]) {
  if (dtype == VM_DTYPE_BF16) {
    Quad<bf16_t> q;
#pragma unroll
    for (int k = 0; k < 4; ++k) q.v[k] = from_f32<bf16_t>(v[k]);
    *reinterpret_cast<Quad<bf16_t>*>(static_cast<bf16_t*>(p) + i) = q;
  } else {
    *reinterpret_cast<float4*>(static_cast<float*>(p) + i) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// The row's statistics in add_norm_vec_kernel / add_norm_kernel's order.  v holds the lane's
// values, 0 where `in` is false.
template <int N>
__device__ __forceinline__ void nb_stats(const float (&v)[N], const bool (&in)[N], int cols,
                                         float eps, int is_rms, float& mean, float& rstd) {
  mean = 0.0f;
  if (is_rms) {
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) sq = fmaf(v[k], v[k], sq);
    rstd = rsqrtf(nb_wave_sum(sq) / cols + eps);
  } else {
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) sum += v[k];
    mean = nb_wave_sum(sum) / cols;
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float dv = in[k] ? v[k] - mean : 0.0f;
      sq = fmaf(dv, dv, sq);
    }
    rstd = rsqrtf(nb_wave_sum(sq) / cols + eps);
  }
}

// Vector form: cols % 4 == 0 and 16-byte aligned buffers.
template <typename S, typename DY, bool DRES, int CPL>
__global__ __launch_bounds__(64) void norm_bwd_vec_kernel(const NormBwdParams p,
                                                          const NormBwdPlan pl,
                                                          float* __restrict__ ws) {
  constexpr int N = CPL * 4;
  const int lane = threadIdx.x, wg = blockIdx.x;
  const long long r0 = pl.row_begin(wg), r1 = pl.row_end(wg, p.rows);
  int col[CPL];
  bool in[N];
  float wv[N], aw[N], ab[N];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    const int c = lane * 4 + 256 * j;
    const bool ok = c < p.cols;
    col[j] = ok ? c : 0;
    const float4 q = *reinterpret_cast<const float4*>(p.w + col[j]);
    wv[4 * j] = q.x; wv[4 * j + 1] = q.y; wv[4 * j + 2] = q.z; wv[4 * j + 3] = q.w;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      in[4 * j + i] = ok;
      aw[4 * j + i] = ab[4 * j + i] = 0.0f;
    }
  }
  const S* sp = static_cast<const S*>(p.s);
  const DY* gp = static_cast<const DY*>(p.dy);
  const S* rp = static_cast<const S*>(p.dres);
  Quad<S> sq[CPL], rq[CPL], sn[CPL], rn[CPL];
  Quad<DY> gq[CPL], gn[CPL];
  auto load_row = [&](long long row, Quad<S> (&a)[CPL], Quad<DY> (&g)[CPL], Quad<S> (&r)[CPL]) {
    const long long base = row * p.cols;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      a[j] = *reinterpret_cast<const Quad<S>*>(sp + base + col[j]);
      g[j] = *reinterpret_cast<const Quad<DY>*>(gp + base + col[j]);
      if constexpr (DRES) r[j] = *reinterpret_cast<const Quad<S>*>(rp + base + col[j]);
    }
  };
  load_row(r0, sn, gn, rn);
  for (long long row = r0; row < r1; ++row) {
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      sq[j] = sn[j];
      gq[j] = gn[j];
      if constexpr (DRES) rq[j] = rn[j];
    }
    load_row(row + 1 < r1 ? row + 1 : row, sn, gn, rn);  // the next row, in flight meanwhile
    float v[N], dyv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      v[k] = in[k] ? to_f32(sq[k >> 2].v[k & 3]) : 0.0f;
      dyv[k] = in[k] ? to_f32(gq[k >> 2].v[k & 3]) : 0.0f;
    }
    float mean, rstd;
    nb_stats<N>(v, in, p.cols, p.eps, p.is_rms, mean, rstd);
    float xh[N], gx = 0.0f, gs = 0.0f;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      xh[k] = in[k] ? (v[k] - mean) * rstd : 0.0f;
      const float g = dyv[k] * wv[k];
      gx = fmaf(g, xh[k], gx);
      gs += g;
      aw[k] = fmaf(dyv[k], xh[k], aw[k]);
      ab[k] += dyv[k];
    }
    const float c1 = nb_wave_sum(gx) / p.cols;
    const float c2 = p.is_rms ? 0.0f : nb_wave_sum(gs) / p.cols;
    const long long base = row * p.cols;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      float ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 4 * j + i;
        ds[i] = rstd * (dyv[k] * wv[k] - c2 - xh[k] * c1);
        if constexpr (DRES) ds[i] += to_f32(rq[j].v[i]);
      }
      if (in[4 * j]) {
        nb_store4(p.dx, base + col[j], p.dx_dtype, ds);
        if (p.dr) nb_store4(p.dr, base + col[j], p.dr_dtype, ds);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    if (!in[4 * j]) continue;
    float* d0 = ws + pl.part_offset(wg, 0) + col[j];
    float* d1 = ws + pl.part_offset(wg, 1) + col[j];
    *reinterpret_cast<float4*>(d0) = make_float4(aw[4 * j], aw[4 * j + 1], aw[4 * j + 2], aw[4 * j + 3]);
    *reinterpret_cast<float4*>(d1) = make_float4(ab[4 * j], ab[4 * j + 1], ab[4 * j + 2], ab[4 * j + 3]);
  }
}

// Any cols, any alignment: lane l holds columns l + 64 j, dtypes read at run time.
template <int VPL>
__global__ __launch_bounds__(64) void norm_bwd_kernel(const NormBwdParams p, const NormBwdPlan pl,
                                                      float* __restrict__ ws) {
  const int lane = threadIdx.x, wg = blockIdx.x;
  const long long r0 = pl.row_begin(wg), r1 = pl.row_end(wg, p.rows);
  int col[VPL];
  bool in[VPL];
  float wv[VPL], aw[VPL], ab[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const int c = lane + 64 * j;
    in[j] = c < p.cols;
    col[j] = in[j] ? c : 0;
    wv[j] = p.w[col[j]];
    aw[j] = ab[j] = 0.0f;
  }
  for (long long row = r0; row < r1; ++row) {
    const long long base = row * p.cols;
    float v[VPL], dyv[VPL], dres[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const float sv = load_dyn(p.s, base + col[j], p.s_dtype);
      const float gv = load_dyn(p.dy, base + col[j], p.dy_dtype);
      dres[j] = p.dres ? load_dyn(p.dres, base + col[j], p.s_dtype) : 0.0f;
      v[j] = in[j] ? sv : 0.0f;
      dyv[j] = in[j] ? gv : 0.0f;
    }
    float mean, rstd;
    nb_stats<VPL>(v, in, p.cols, p.eps, p.is_rms, mean, rstd);
    float xh[VPL], gx = 0.0f, gs = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      xh[j] = in[j] ? (v[j] - mean) * rstd : 0.0f;
      const float g = dyv[j] * wv[j];
      gx = fmaf(g, xh[j], gx);
      gs += g;
      aw[j] = fmaf(dyv[j], xh[j], aw[j]);
      ab[j] += dyv[j];
    }
    const float c1 = nb_wave_sum(gx) / p.cols;
    const float c2 = p.is_rms ? 0.0f : nb_wave_sum(gs) / p.cols;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      const float ds = rstd * (dyv[j] * wv[j] - c2 - xh[j] * c1) + dres[j];
      if (in[j]) {
        store_dyn(p.dx, base + col[j], p.dx_dtype, ds);
        if (p.dr) store_dyn(p.dr, base + col[j], p.dr_dtype, ds);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    if (!in[j]) continue;
    ws[pl.part_offset(wg, 0) + col[j]] = aw[j];
    ws[pl.part_offset(wg, 1) + col[j]] = ab[j];
  }
}

// dweight | dbias: thread (column, range) adds its range of workgroups in order, then the
// range sums are added in range order.  grid (cpad / 64, 2), 64 x kNbRanges threads.
__global__ __launch_bounds__(64 * kNbRanges) void norm_bwd_reduce_kernel(
    const NormBwdParams p, const NormBwdPlan pl, const float* __restrict__ ws) {
  __shared__ float sums[kNbRanges][64];
  const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;  // < cpad
  const int which = blockIdx.y;
  float acc = 0.0f;
  const int we = pl.range_end(r);
  // columns in [cols, cpad) were never written: read and dropped below
  for (int g = pl.range_begin(r); g < we; ++g) acc += ws[pl.part_offset(g, which) + col];
  sums[r][c] = acc;
  __syncthreads();
  if (r != 0 || col >= p.cols) return;
  float total = 0.0f;
#pragma unroll
  for (int k = 0; k < kNbRanges; ++k) total += sums[k][c];
  if (which == 0) p.dw[col] = total;
  else if (p.db) p.db[col] = total;
}

template <typename S, typename DY, bool DRES>
static void launch_norm_bwd_vec(const NormBwdParams& p, const NormBwdPlan& pl, float* ws,
                                hipStream_t s) {
  const dim3 grid(pl.nwg), block(64);
  const int cpl = (p.cols + 255) / 256;
  if (cpl <= 1) hipLaunchKernelGGL((norm_bwd_vec_kernel<S, DY, DRES, 1>), grid, block, 0, s, p, pl, ws);
  else if (cpl <= 2) hipLaunchKernelGGL((norm_bwd_vec_kernel<S, DY, DRES, 2>), grid, block, 0, s, p, pl, ws);
  else if (cpl <= 4) hipLaunchKernelGGL((norm_bwd_vec_kernel<S, DY, DRES, 4>), grid, block, 0, s, p, pl, ws);
  else hipLaunchKernelGGL((norm_bwd_vec_kernel<S, DY, DRES, 8>), grid, block, 0, s, p, pl, ws);
}

template <typename S, typename DY>
static void dispatch_norm_bwd_vec(const NormBwdParams& p, const NormBwdPlan& pl, float* ws,
                                  hipStream_t s) {
  if (p.dres) launch_norm_bwd_vec<S, DY, true>(p, pl, ws, s);
  else launch_norm_bwd_vec<S, DY, false>(p, pl, ws, s);
}

}  // namespace vm

using namespace vm;

extern "C" long long vm_add_norm_bwd_workspace_bytes(long long rows, int cols) {
  if (cols > kNbMaxCols) return 0;
  return static_cast<long long>(plan_norm_bwd(rows, cols).ws_bytes);
}

extern "C" int vm_add_norm_bwd(const void* s, int s_dtype, const float* weight,
                               const float* bias, const void* dy, int dy_dtype,
                               const void* dres_out, void* dx, int dx_dtype, void* dresidual,
                               int dres_dtype, float* dweight, float* dbias, long long rows,
                               int cols, float eps, int is_rms, void* workspace,
                               long long workspace_bytes, vm_stream_t stream) {
  const char* name = "vm_add_norm_bwd";
  if (!s || !weight || !dy || !dx || !dweight) {
    vmhost::set_error("%s: null required pointer (s, weight, dy, dx, dweight)", name);
    return VM_E_INVALID;
  }
  if ((bias != nullptr) != (dbias != nullptr)) {
    vmhost::set_error("%s: dbias goes with the norm's bias (both or neither)", name);
    return VM_E_INVALID;
  }
  if (rows < 0 || cols < 1 || cols > kNbMaxCols) {
    vmhost::set_error("%s: bad shape rows=%lld cols=%d (cols must be in [1, %d])", name, rows,
                      cols, kNbMaxCols);
    return VM_E_INVALID;
  }
  if (!vmhost::dtype_ok(s_dtype) || !vmhost::dtype_ok(dy_dtype) || !vmhost::dtype_ok(dx_dtype) ||
      (dresidual && !vmhost::dtype_ok(dres_dtype))) {
    vmhost::set_error("%s: unsupported dtype", name);
    return VM_E_INVALID;
  }
  const NormBwdPlan pl = plan_norm_bwd(rows, cols);
  if (pl.ws_bytes > 0 &&
      (!workspace || workspace_bytes < static_cast<long long>(pl.ws_bytes))) {
    vmhost::set_error("%s: workspace of %lld bytes, need %zu (vm_add_norm_bwd_workspace_bytes)",
                      name, workspace ? workspace_bytes : 0ll, pl.ws_bytes);
    return VM_E_INVALID;
  }
  NormBwdParams p{};
  p.s = s; p.w = weight; p.dy = dy; p.dres = dres_out; p.dx = dx; p.dr = dresidual;
  p.dw = dweight; p.db = dbias; p.rows = rows; p.cols = cols; p.eps = eps; p.is_rms = is_rms;
  p.s_dtype = s_dtype; p.dy_dtype = dy_dtype; p.dx_dtype = dx_dtype; p.dr_dtype = dres_dtype;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  if (pl.nwg > 0) {
    const bool vec = cols % 4 == 0 && vmhost::aligned16(s) && vmhost::aligned16(dy) &&
                     vmhost::aligned16(dx) && vmhost::aligned16(weight) && vmhost::aligned16(ws) &&
                     (!dres_out || vmhost::aligned16(dres_out)) &&
                     (!dresidual || vmhost::aligned16(dresidual));
    if (vec) {
      const bool sb = s_dtype == VM_DTYPE_BF16, gb = dy_dtype == VM_DTYPE_BF16;
      if (sb && gb) dispatch_norm_bwd_vec<bf16_t, bf16_t>(p, pl, ws, st);
      else if (sb) dispatch_norm_bwd_vec<bf16_t, float>(p, pl, ws, st);
      else if (gb) dispatch_norm_bwd_vec<float, bf16_t>(p, pl, ws, st);
      else dispatch_norm_bwd_vec<float, float>(p, pl, ws, st);
    } else {
      const dim3 grid(pl.nwg), block(64);
      const int vpl = (cols + 63) / 64;
      if (vpl <= 4) hipLaunchKernelGGL(norm_bwd_kernel<4>, grid, block, 0, st, p, pl, ws);
      else if (vpl <= 8) hipLaunchKernelGGL(norm_bwd_kernel<8>, grid, block, 0, st, p, pl, ws);
      else if (vpl <= 16) hipLaunchKernelGGL(norm_bwd_kernel<16>, grid, block, 0, st, p, pl, ws);
      else hipLaunchKernelGGL(norm_bwd_kernel<32>, grid, block, 0, st, p, pl, ws);
    }
  }
  hipLaunchKernelGGL(norm_bwd_reduce_kernel, dim3(pl.cpad / 64, 2), dim3(64 * kNbRanges), 0, st,
                     p, pl, ws);
  return vmhost::launch_status(name);
}

// Backward of the token-major depthwise causal conv1d (+bias, SiLU): the gradient of
// vm_causal_conv1d_fwd from the forward's inputs alone.  With e = [cs_in | x] the virtual
// input,
//   pre[t]  = bias + sum_i w[i] e[t - width + 1 + i]      (recomputed, the forward's fma order)
//   dpre[t] = dout[t] silu'(pre[t])                        (dout[t] without SiLU)
//   de[j]   = sum_i w[i] dpre[j + width - 1 - i]           (steps that exist)
//   dw[i]   = sum_{b,t} dpre[t] e[t - width + 1 + i],  dbias = sum_{b,t} dpre[t]
// all in fp32; dx is rounded once at the store.
//
// conv_bwd_kernel follows conv_tm_kernel: a thread owns CPT adjacent channels (a 16-byte
// run), walks a time tile forwards and keeps the last kCbWM rows of e and of dpre in
// registers.  de[j] is complete once dpre[j + kCbWM - 1] is known, so the walk runs
// kCbWM - 1 steps past the tile's end and stores dx three steps behind its loads: every row
// of x and dout is read once per tile plus that halo.  Taps are right-aligned in kCbWM slots,
// the missing leading ones zero, as in the forward.  The tile's dw / dbias sums go to the
// workspace (vm_conv_bwd_plan.h); conv_bwd_reduce_kernel adds them in a fixed order.  No
// atomics.
//
// Bounds: the row index of every load is clamped into [0, seqlen) and dout past the
// sequence is used as 0, the channel group of a thread past `dim` is clamped to the last one
// and that thread stores nothing — no load sits under a lane-dependent branch.

#include "vm_common.h"
#include "vm_conv_bwd_plan.h"

namespace vm {

struct ConvBwdParams {
  const void* x; const float* w; const float* bias; const void* csi; const void* dout;
  void* dx; float* dcs; float* dw; float* db;
  long long x_sb, x_sl, csi_sb, csi_sd, do_sb, do_sl, dx_sb, dx_sl, dcs_sb, dcs_sd;
  int batch, dim, seqlen, width, silu, csi_dtype;
};

// CPT adjacent elements moved as one access
template <typename T, int CPT>
struct alignas(sizeof(T) * CPT) Run {
  T v[CPT];
};

__device__ __forceinline__ float dsilu(float x) {
  const float sg = 1.0f / (1.0f + __expf(-x));
  return sg * fmaf(x, 1.0f - sg, 1.0f);
}

template <typename T, int CPT>
__global__ __launch_bounds__(64) void conv_bwd_kernel(const ConvBwdParams p, const ConvBwdPlan pl,
                                                      float* __restrict__ ws) {
  constexpr int WM = kCbWM;
  typedef Run<T, CPT> RunT;
  const int ngroups = p.dim / CPT;  // dim % CPT == 0 (dispatch)
  const int g = blockIdx.x * kCbLanes + threadIdx.x;
  const bool live = g < ngroups;
  const int d0 = (live ? g : ngroups - 1) * CPT;
  const int b = blockIdx.z, tile = blockIdx.y;
  const int W = p.width, L = p.seqlen;
  const int t0 = pl.tile_begin(tile), t1 = pl.tile_end(tile, L);
  const T* __restrict__ xb = static_cast<const T*>(p.x) + b * p.x_sb + d0;
  const T* __restrict__ gb = static_cast<const T*>(p.dout) + b * p.do_sb + d0;
  T* __restrict__ ob = static_cast<T*>(p.dx) + b * p.dx_sb + d0;

  float w[WM][CPT], bias[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
#pragma unroll
    for (int k = 0; k < WM; ++k) {  // right-aligned taps: w[WM-1] multiplies e[t]
      const int i = k - (WM - W);
      w[k][c] = i >= 0 ? p.w[(d0 + c) * W + i] : 0.0f;
    }
    bias[c] = p.bias ? p.bias[d0 + c] : 0.0f;
  }

  float hist[WM][CPT];  // hist[k] = e[t - (WM-1) + k], k = WM-1 is the current row
  float dwin[WM][CPT];  // dwin[k] = dpre[t - (WM-1) + k]
  float aw[WM][CPT], ab[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    ab[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < WM; ++k) aw[k][c] = dwin[k][c] = hist[k][c] = 0.0f;
  }
  if (t0 > 0) {  // t0 >= kCbTT > WM: the rows before the tile are rows of x
#pragma unroll
    for (int k = 0; k < WM - 1; ++k) {
      const RunT r = *reinterpret_cast<const RunT*>(xb + (t0 - (WM - 1) + k) * p.x_sl);
#pragma unroll
      for (int c = 0; c < CPT; ++c) hist[k][c] = to_f32(r.v[c]);
    }
  } else if (p.csi) {  // e[j] = cs_in[W + j] for -W <= j < 0
#pragma unroll
    for (int k = 0; k < WM - 1; ++k) {
      const int slot = W - (WM - 1) + k;
#pragma unroll
      for (int c = 0; c < CPT; ++c)
        hist[k][c] = slot >= 0 ? load_dyn(p.csi, b * p.csi_sb + (d0 + c) * p.csi_sd + slot,
                                          p.csi_dtype)
                               : 0.0f;
    }
  }

  const int t_stop = t1 + WM - 1;  // dx[t1 - 1] is complete after step t1 + WM - 2
  const int tmax = L - 1;
  for (int tb = t0; tb < t_stop; tb += 8) {
    RunT xr[8], gr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int tc = tb + i < tmax ? tb + i : tmax;
      xr[i] = *reinterpret_cast<const RunT*>(xb + tc * p.x_sl);
      gr[i] = *reinterpret_cast<const RunT*>(gb + tc * p.do_sl);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = tb + i;
      const bool own = t < t1;  // the tile's own steps feed dw / dbias
      float de[CPT];
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        hist[WM - 1][c] = to_f32(xr[i].v[c]);
        float pre = bias[c];
#pragma unroll
        for (int k = 0; k < WM; ++k) pre = fmaf(w[k][c], hist[k][c], pre);
        float dp = t < L ? to_f32(gr[i].v[c]) : 0.0f;
        if (p.silu) dp *= dsilu(pre);
        dwin[WM - 1][c] = dp;
        const float dpo = own ? dp : 0.0f;
        ab[c] += dpo;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < WM; ++k) {
          aw[k][c] = fmaf(dpo, hist[k][c], aw[k][c]);
          acc = fmaf(w[k][c], dwin[WM - 1 - k][c], acc);
        }
        de[c] = acc;
      }
      const int j = t - (WM - 1);
      if (j >= t0 && j < t1 && live) {
        RunT o;
#pragma unroll
        for (int c = 0; c < CPT; ++c) o.v[c] = from_f32<T>(de[c]);
        *reinterpret_cast<RunT*>(ob + j * p.dx_sl) = o;
      }
      if (j < 0 && W + j >= 1 && p.dcs && live) {  // tile 0: the gradient of cs_in[W + j]
#pragma unroll
        for (int c = 0; c < CPT; ++c)
          p.dcs[b * p.dcs_sb + (d0 + c) * p.dcs_sd + W + j] = de[c];
      }
#pragma unroll
      for (int k = 0; k < WM - 1; ++k)
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
          hist[k][c] = hist[k + 1][c];
          dwin[k][c] = dwin[k + 1][c];
        }
    }
  }
  if (!live) return;
  if (tile == 0 && p.dcs) {  // no tap reaches the oldest state entry
#pragma unroll
    for (int c = 0; c < CPT; ++c) p.dcs[b * p.dcs_sb + (d0 + c) * p.dcs_sd] = 0.0f;
  }
  const long long part = static_cast<long long>(b) * pl.tiles + tile;
#pragma unroll
  for (int k = 0; k < WM; ++k) {
    const int i = k - (WM - W);
    if (i < 0) continue;
    float* dst = ws + pl.part_offset(part, i) + d0;
#pragma unroll
    for (int c = 0; c < CPT; ++c) dst[c] = aw[k][c];
  }
  float* dst = ws + pl.part_offset(part, W) + d0;
#pragma unroll
  for (int c = 0; c < CPT; ++c) dst[c] = ab[c];
}

// dweight | dbias: thread (channel, range) adds its range of parts in index order, then the
// range sums are added in range order.  grid (dpad / 64, width + 1), 64 x kCbRanges threads.
// Without any part (an empty sequence) the sums are 0 and so is dcs_in.
__global__ __launch_bounds__(kCbLanes * kCbRanges) void conv_bwd_reduce_kernel(
    const ConvBwdParams p, const ConvBwdPlan pl, const float* __restrict__ ws) {
  __shared__ float sums[kCbRanges][kCbLanes];
  const int c = threadIdx.x & (kCbLanes - 1), r = threadIdx.x / kCbLanes;
  const int d = blockIdx.x * kCbLanes + c;  // < dpad
  const int slot = blockIdx.y;
  float acc = 0.0f;
  const long long pe = pl.range_end(r);
  for (long long i = pl.range_begin(r); i < pe; ++i) acc += ws[pl.part_offset(i, slot) + d];
  sums[r][c] = acc;
  __syncthreads();
  if (r != 0 || d >= p.dim) return;
  float total = 0.0f;
#pragma unroll
  for (int k = 0; k < kCbRanges; ++k) total += sums[k][c];
  if (slot < p.width) p.dw[d * p.width + slot] = total;
  else if (p.db) p.db[d] = total;
  if (slot == 0 && pl.parts == 0 && p.dcs) {
    for (int b = 0; b < p.batch; ++b)
      for (int k = 0; k < p.width; ++k) p.dcs[b * p.dcs_sb + d * p.dcs_sd + k] = 0.0f;
  }
}

template <typename T, int CPT>
static void launch_conv_bwd(const ConvBwdParams& p, const ConvBwdPlan& pl, float* ws,
                            hipStream_t s) {
  if (pl.parts > 0) {
    const int groups = p.dim / CPT;
    dim3 grid((groups + kCbLanes - 1) / kCbLanes, pl.tiles, p.batch);
    hipLaunchKernelGGL((conv_bwd_kernel<T, CPT>), grid, dim3(kCbLanes), 0, s, p, pl, ws);
  }
  hipLaunchKernelGGL(conv_bwd_reduce_kernel, dim3(pl.dpad / kCbLanes, pl.slots),
                     dim3(kCbLanes * kCbRanges), 0, s, p, pl, ws);
}

template <typename T>
static void dispatch_conv_bwd(const ConvBwdParams& p, const ConvBwdPlan& pl, float* ws,
                              hipStream_t s) {
  const long long es = sizeof(T);
  auto ok = [&](int cpt) {
    const long long bytes = cpt * es;
    auto al = [&](const void* q, long long sb, long long sl) {
      return reinterpret_cast<uintptr_t>(q) % bytes == 0 && (sb * es) % bytes == 0 &&
             (sl * es) % bytes == 0;
    };
    return p.dim % cpt == 0 && al(p.x, p.x_sb, p.x_sl) && al(p.dout, p.do_sb, p.do_sl) &&
           al(p.dx, p.dx_sb, p.dx_sl);
  };
  if constexpr (sizeof(T) == 2) {
    if (ok(8)) return launch_conv_bwd<T, 8>(p, pl, ws, s);
  }
  if (ok(4)) launch_conv_bwd<T, 4>(p, pl, ws, s);
  else launch_conv_bwd<T, 1>(p, pl, ws, s);
}

}  // namespace vm

using namespace vm;

extern "C" long long vm_causal_conv1d_bwd_workspace_bytes(int batch, int dim, int seqlen,
                                                          int width) {
  return static_cast<long long>(plan_conv_bwd(batch, dim, seqlen, width).ws_bytes);
}

extern "C" int vm_causal_conv1d_bwd(
    const void* x, long long x_sb, long long x_sd, long long x_sl, const float* weight,
    const float* bias, const void* cs_in, int cs_in_dtype, long long csi_sb, long long csi_sd,
    const void* dout, long long do_sb, long long do_sd, long long do_sl,
    void* dx, long long dx_sb, long long dx_sd, long long dx_sl,
    float* dcs_in, long long dcs_sb, long long dcs_sd, float* dweight, float* dbias,
    int batch, int dim, int seqlen, int width, int silu, int dtype,
    void* workspace, long long workspace_bytes, vm_stream_t stream) {
  const char* name = "vm_causal_conv1d_bwd";
  if (!x || !weight || !dout || !dx || !dweight) {
    vmhost::set_error("%s: null required pointer (x, weight, dout, dx, dweight)", name);
    return VM_E_INVALID;
  }
  if ((bias != nullptr) != (dbias != nullptr)) {
    vmhost::set_error("%s: dbias goes with bias (both or neither)", name);
    return VM_E_INVALID;
  }
  if (batch < 0 || dim < 0 || seqlen < 0 || width < 1 || width > kCbWM) {
    vmhost::set_error("%s: bad shape batch=%d dim=%d seqlen=%d width=%d (width must be in "
                      "[1, %d])", name, batch, dim, seqlen, width, kCbWM);
    return VM_E_INVALID;
  }
  if (!vmhost::dtype_ok(dtype) || (cs_in && !vmhost::dtype_ok(cs_in_dtype))) {
    vmhost::set_error("%s: unsupported dtype", name);
    return VM_E_INVALID;
  }
  if (dim > 1 && (x_sd != 1 || do_sd != 1 || dx_sd != 1)) {
    vmhost::set_error("%s: token-major operands only: x / dout / dx need a unit channel stride",
                      name);
    return VM_E_INVALID;
  }
  const ConvBwdPlan pl = plan_conv_bwd(batch, dim, seqlen, width);
  if (pl.ws_bytes > 0 &&
      (!workspace || workspace_bytes < static_cast<long long>(pl.ws_bytes))) {
    vmhost::set_error("%s: workspace of %lld bytes, need %zu "
                      "(vm_causal_conv1d_bwd_workspace_bytes)", name,
                      workspace ? workspace_bytes : 0ll, pl.ws_bytes);
    return VM_E_INVALID;
  }
  if (dim == 0) return VM_OK;
  ConvBwdParams p{};
  p.x = x; p.w = weight; p.bias = bias; p.csi = cs_in; p.dout = dout;
  p.dx = dx; p.dcs = dcs_in; p.dw = dweight; p.db = dbias;
  p.x_sb = x_sb; p.x_sl = x_sl; p.csi_sb = csi_sb; p.csi_sd = csi_sd;
  p.do_sb = do_sb; p.do_sl = do_sl; p.dx_sb = dx_sb; p.dx_sl = dx_sl;
  p.dcs_sb = dcs_sb; p.dcs_sd = dcs_sd;
  p.batch = batch; p.dim = dim; p.seqlen = seqlen; p.width = width; p.silu = silu;
  p.csi_dtype = cs_in_dtype;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == VM_DTYPE_BF16) dispatch_conv_bwd<bf16_t>(p, pl, static_cast<float*>(workspace), s);
  else dispatch_conv_bwd<float>(p, pl, static_cast<float*>(workspace), s);
  return vmhost::launch_status(name);
}

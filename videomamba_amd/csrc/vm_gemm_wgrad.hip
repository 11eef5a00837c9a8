// Weight gradient of the projection GEMM: dw[n, k] = sum over m of dy[m, n] * x[m, k], bf16
// operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, dw stored in bf16 or fp32 (rounded
// once, at the store).  The reduction runs over the ROW index of both operands, so both are
// staged into LDS as they lie in memory (rows of m, contiguous in the column) and both MFMA
// operands are read with the gfx950 transposed LDS read, ds_read_b64_tr_b16.
//
// Two kernels (geometry: vm_gemm_wgrad_plan.h):
//   wgrad_partial_kernel  one workgroup per (128 x 128 output tile, slice of m): fp32 partial
//                         tile -> part[slice][n][k]
//   wgrad_reduce_kernel   adds the slices of every element in slice order, rounds, stores dw
// No atomics, and the slicing is a function of (m, n, k) alone: dw has the same bits on any
// device and on a second call.

#include "vm_common.h"
#include "vm_gemm_wgrad_plan.h"

namespace vm {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short wg_bf16x8_t;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float wg_f32x4_t;

struct WgradParams {
  const bf16_t* dy; long long lddy;  // (m, n)
  const bf16_t* x; long long ldx;    // (m, k)
  float* part;                       // [slices][n][k]
  int m, n, k;
  int slice_rows;
};

// LDS image of one operand's stage: kWgStageRows rows of 256 bytes (128 bf16 columns), the
// 16-byte chunk ch of row r at slot ch ^ wg_xor(r) (cdna_hip_programming.md T10, image (b)).
// A 32-lane half of a transposed read takes two 4-row blocks 8 rows apart in the same 16
// columns: rows r and r + 8 differ in bit 1 of the XOR (the other 32-byte pair of a 64-byte
// segment), the 4 rows of a block in bits 2-3 (the four segments), so the half's 32 lanes
// touch each of the 64 banks once.  Without the XOR the eight rows would share 32 bytes of
// the bank row (8-way).  The XOR may swap the two chunks of a block row's 32 bytes, so every
// address goes through wg_off.
__device__ __forceinline__ int wg_xor(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int wg_off(int row, int ch) {
  return kWgRowBytes * row + 16 * (ch ^ wg_xor(row));
}
constexpr int kWgOob = 0x7ffffff0;  // past every buffer range (ranges are under 2^31): reads 0

// s_waitcnt vmcnt(N) lgkmcnt(0) (expcnt left at its maximum)
template <int N>
__device__ __forceinline__ void wg_wait_vm_lgkm0() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | 0x0070);
}

// One transposed read: the 16-lane group of this lane gets a block of 4 rows x 16 columns,
// lane i of the group column i, row q in element q.  `addr` is this lane's Mechanism address
// (row q = (lane >> 2) & 3 of the block, columns 4 (lane & 3) ...) as an LDS byte address,
// 8-byte aligned.  EXEC is all ones at every call: the kernel has no divergent branch around
// it and 256 threads.  Inline assembly, not the builtin: hipcc orders an LDS read it can see
// behind every outstanding LDS-DMA load (s_waitcnt vmcnt(0) in front of each stage's reads),
// which would leave no stage in flight; the kernel counts vmcnt itself.  hipcc does not count
// lgkmcnt for these either: wg_tr_wait() stands between the reads and their first use.
typedef __attribute__((__vector_size__(2 * sizeof(int)))) int wg_i32x2_t;
typedef __attribute__((__vector_size__(4 * sizeof(int)))) int wg_i32x4_t;
__device__ __forceinline__ wg_i32x2_t wg_tr_read(int addr) {
  wg_i32x2_t v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}
__device__ __forceinline__ void wg_tr_wait(wg_i32x4_t (&a)[4], wg_i32x4_t (&b)[4]) {
  asm volatile("s_waitcnt lgkmcnt(0)"
               : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]),
                 "+v"(b[2]), "+v"(b[3])
               :
               : "memory");
}

__global__ __launch_bounds__(kWgThreads) void wgrad_partial_kernel(const WgradParams p) {
  constexpr int R = kWgRowBytes;
  constexpr int RB = kWgStageRows;
  constexpr int NBUF = kWgStages;
  constexpr int OPER = RB * R;       // bytes of one operand's stage image
  constexpr int STAGE = 2 * OPER;    // [dy image | x image]
  constexpr int NW = kWgThreads / 64;
  constexpr int GI = OPER / (1024 * NW);  // DMA instructions per wave per operand per stage
  constexpr int G = 2 * GI;
  static_assert(GI * 1024 * NW == OPER, "a stage image must fill whole DMA rounds");
  static_assert(RB == 32, "one 16x16x32 MFMA step per stage");
  static_assert(kWgTileN == 128 && kWgTileK == 128 && NW == 4, "2 x 2 waves of 64 x 64");
  static_assert((NBUF - 2) * G < 64, "vmcnt is 6 bits");
  extern __shared__ __attribute__((aligned(16))) char dsm[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int k0 = blockIdx.x * kWgTileK, n0 = blockIdx.y * kWgTileN;
  const int slice = blockIdx.z;
  const int s_beg = slice * p.slice_rows;
  const int s_end = min(p.m, s_beg + p.slice_rows);
  const int nsteps = (s_end - s_beg + RB - 1) / RB;

  // rows [0, m) of each operand through one buffer: the last row ends at its width
  const auto dyr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(p.dy), 0,
      static_cast<int>(((long long)(p.m - 1) * p.lddy + p.n) * 2), 0x00020000);
  const auto xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16_t*>(p.x), 0,
      static_cast<int>(((long long)(p.m - 1) * p.ldx + p.k) * 2), 0x00020000);

  // Per-lane source of this wave's DMA instructions.  Instruction t of an operand fills LDS
  // rows 4 t ... 4 t + 3 of the image lane-linearly: lane l writes slot l & 15 of row
  // 4 t + (l >> 4), which holds chunk (l & 15) ^ wg_xor(row).  Columns past the operand's
  // width and rows past the slice read as zero: an offset past the buffer, never a branch.
  int drow[GI], dcol_dy[GI], dcol_x[GI];
#pragma unroll
  for (int i = 0; i < GI; ++i) {
    const int t = wave * GI + i;
    const int row = 4 * t + (lane >> 4);
    const int ch = (lane & 15) ^ wg_xor(row);
    drow[i] = row;
    dcol_dy[i] = n0 + 8 * ch < p.n ? (n0 + 8 * ch) * 2 : -1;
    dcol_x[i] = k0 + 8 * ch < p.k ? (k0 + 8 * ch) * 2 : -1;
  }
  auto issue = [&](int step, int buf) {
    char* sd = dsm + buf * STAGE;
    char* sx = sd + OPER;
    const int r0 = s_beg + step * RB;
#pragma unroll
    for (int i = 0; i < GI; ++i) {
      const int row = r0 + drow[i];
      const bool live = row < s_end;
      const int od = live && dcol_dy[i] >= 0
                         ? row * static_cast<int>(p.lddy) * 2 + dcol_dy[i] : kWgOob;
      const int ox = live && dcol_x[i] >= 0
                         ? row * static_cast<int>(p.ldx) * 2 + dcol_x[i] : kWgOob;
      dma16(dyr, sd + (wave * GI + i) * 1024, od);
      dma16(xr, sx + (wave * GI + i) * 1024, ox);
    }
  };

  // Transposed-read addresses inside an operand image.  Group g = lane >> 4 reads rows
  // 8 g ... 8 g + 3 (first read) and 8 g + 4 ... 8 g + 7 (second) of the stage, so fragment
  // element j is row 8 g + j: the MFMA's k index 8 (lane >> 4) + j, for A and B alike.
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  int aad[4][2], bad[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * g + 4 * h + q;
      const int ca = wn * 8 + 2 * i + (pp >> 1), cb = wk * 8 + 2 * i + (pp >> 1);
      aad[i][h] = wg_off(row, ca) + 8 * (pp & 1);
      bad[i][h] = OPER + wg_off(row, cb) + 8 * (pp & 1);
    }

  wg_f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = wg_f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int lds0 = static_cast<int>(reinterpret_cast<uintptr_t>(
      (__attribute__((address_space(3))) char*)dsm));
  auto compute = [&](int buf) {
    const int st = lds0 + buf * STAGE;
    wg_i32x4_t af[4], bf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const wg_i32x2_t a0 = wg_tr_read(st + aad[i][0]), a1 = wg_tr_read(st + aad[i][1]);
      const wg_i32x2_t b0 = wg_tr_read(st + bad[i][0]), b1 = wg_tr_read(st + bad[i][1]);
      af[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3);
      bf[i] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3);
    }
    wg_tr_wait(af, bf);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(wg_bf16x8_t, af[i]), __builtin_bit_cast(wg_bf16x8_t, bf[j]),
            acc[i][j], 0, 0, 0);
  };

  // NBUF - 1 stages in flight across the raw barrier (the forward's LDS-DMA pipeline,
  // vm_gemm.hip).  Every iteration issues a stage, past the slice's end one of zeros into a
  // buffer nobody reads again, so the counted vmcnt is the same constant in every iteration.
#pragma unroll
  for (int s = 0; s < NBUF - 1; ++s) issue(s, s);
  // (unrolled by NBUF so that every stage buffer is a compile-time offset)
#pragma unroll 1
  for (int step0 = 0; step0 < nsteps; step0 += NBUF) {
#pragma unroll
    for (int buf = 0; buf < NBUF; ++buf) {
      const int step = step0 + buf;
      if (step >= nsteps) break;  // uniform
      // stage `step` (this wave's share) has landed once at most the NBUF - 2 stages issued
      // after it are outstanding; the barrier covers every wave's share, and every wave is
      // past its reads (lgkmcnt(0)) of the buffer the issue below refills (stage step - 1's)
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      wg_wait_vm_lgkm0<(NBUF - 2) * G>();
      __builtin_amdgcn_s_barrier();
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
      issue(step + NBUF - 1, (buf + NBUF - 1) % NBUF);
      compute(buf);
    }
  }
  // the trailing zero stages land in LDS before the workgroup's LDS is released
  __builtin_amdgcn_s_waitcnt(0);

  // D[4 (lane / 16) + r][lane % 16] of every 16 x 16 block: row = n, column = k
  float* part = p.part + static_cast<size_t>(slice) * p.n * p.k;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kc = k0 + wk * 64 + j * 16 + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nr = n0 + wn * 64 + i * 16 + (lane >> 4) * 4 + r;
        if (nr < p.n && kc < p.k) part[static_cast<size_t>(nr) * p.k + kc] = acc[i][j][r];
      }
    }
}

// One thread per 4 consecutive columns of one row of dw: adds part[0 .. slices) in slice
// order (slices == 0: zeros) and rounds once to dw's dtype.
template <typename T>
__global__ __launch_bounds__(kWgReduceThreads) void wgrad_reduce_kernel(
    const float* __restrict__ part, T* __restrict__ dw, long long lddw, int n, int k, int slices) {
  const long long id = static_cast<long long>(blockIdx.x) * kWgReduceThreads + threadIdx.x;
  const int kq = k / 4;
  if (id >= static_cast<long long>(n) * kq) return;
  const int row = static_cast<int>(id / kq), c = static_cast<int>(id % kq) * 4;
  const size_t nk = static_cast<size_t>(n) * k;
  const size_t o = static_cast<size_t>(row) * k + c;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < slices; ++i) {
    const float4 v = *reinterpret_cast<const float4*>(part + i * nk + o);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  T* d = dw + row * lddw + c;
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<float4*>(d) = s;
  } else {
    const uint32_t lo = static_cast<uint32_t>(from_f32<bf16_t>(s.x)) |
                        (static_cast<uint32_t>(from_f32<bf16_t>(s.y)) << 16);
    const uint32_t hi = static_cast<uint32_t>(from_f32<bf16_t>(s.z)) |
                        (static_cast<uint32_t>(from_f32<bf16_t>(s.w)) << 16);
    *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
  }
}

static int wgrad_refuse(WgradWhy why, const WgradPlanIn& in, const WgradPlan& pl) {
  switch (why) {
    case WgradWhy::kOk: return VM_OK;
    case WgradWhy::kDtype:
      vmhost::set_error("vm_linear_wgrad: bf16 dy and x only; dw in bf16 or fp32");
      break;
    case WgradWhy::kShape:
      vmhost::set_error("vm_linear_wgrad: m >= 0, n a multiple of 8, k a multiple of 64, "
                        "n * k under 2^29 (m %d, n %d, k %d)", in.m, in.n, in.k);
      break;
    case WgradWhy::kStrides:
      vmhost::set_error("vm_linear_wgrad: leading dimensions at least the width and multiples "
                        "of 8 (lddy %lld, ldx %lld, lddw %lld)", in.lddy, in.ldx, in.lddw);
      break;
    case WgradWhy::kAlign:
      vmhost::set_error("vm_linear_wgrad: dy, x, dw and the workspace must be 16-byte aligned");
      break;
    case WgradWhy::kPast2GB:
      vmhost::set_error("vm_linear_wgrad: dy and x go through one 31-bit buffer each: "
                        "m * ld * 2 must be under 2 GB");
      break;
    case WgradWhy::kWorkspace:
      vmhost::set_error("vm_linear_wgrad: workspace of %lld bytes, "
                        "vm_linear_wgrad_workspace_bytes(m, n, k) is %lld",
                        in.workspace_bytes, pl.workspace_bytes);
      break;
  }
  return VM_E_INVALID;
}

}  // namespace vm

using namespace vm;

extern "C" long long vm_linear_wgrad_workspace_bytes(int m, int n, int k) {
  return plan_linear_wgrad_shape(m, n, k).workspace_bytes;
}

extern "C" long long vm_linear_wgrad_slice_rows(int m, int n, int k) {
  return plan_linear_wgrad_shape(m, n, k).slice_rows;
}

extern "C" int vm_linear_fn_fits(int m, int n, int k) {
  return linear_fn_fits(m, n, k, vmhost::device_cus(nullptr)) ? 1 : 0;
}

extern "C" int vm_linear_wgrad(const void* dy, long long lddy, const void* x, long long ldx,
                               void* dw, long long lddw, int dw_dtype, int m, int n, int k,
                               int dtype, void* workspace, long long workspace_bytes,
                               vm_stream_t stream) {
  WgradPlanIn in{};
  in.m = m; in.n = n; in.k = k; in.lddy = lddy; in.ldx = ldx; in.lddw = lddw;
  in.bf16 = dtype == VM_DTYPE_BF16;
  in.dw_dtype_ok = vmhost::dtype_ok(dw_dtype);
  in.dy_al = vmhost::aligned16(dy); in.x_al = vmhost::aligned16(x);
  in.dw_al = vmhost::aligned16(dw); in.ws_al = vmhost::aligned16(workspace);
  in.workspace_bytes = workspace ? workspace_bytes : 0;
  const WgradPlan pl = plan_linear_wgrad(in);
  if (pl.why != WgradWhy::kOk) return wgrad_refuse(pl.why, in, pl);
  if (!dw || (!pl.empty && (!dy || !x))) {
    vmhost::set_error("vm_linear_wgrad: null required pointer");
    return VM_E_INVALID;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!pl.empty) {
    WgradParams p{};
    p.dy = static_cast<const bf16_t*>(dy); p.lddy = lddy;
    p.x = static_cast<const bf16_t*>(x); p.ldx = ldx;
    p.part = static_cast<float*>(workspace);
    p.m = m; p.n = n; p.k = k;
    p.slice_rows = static_cast<int>(pl.slice_rows);
    hipLaunchKernelGGL(wgrad_partial_kernel, dim3(pl.gx, pl.gy, pl.gz), dim3(pl.block), pl.lds,
                       s, p);
  }
  const int slices = pl.empty ? 0 : pl.slices;
  const float* part = static_cast<const float*>(workspace);
  if (dw_dtype == VM_DTYPE_BF16)
    hipLaunchKernelGGL(wgrad_reduce_kernel<bf16_t>, dim3(pl.rgx), dim3(pl.rblock), 0, s, part,
                       static_cast<bf16_t*>(dw), lddw, n, k, slices);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<float>, dim3(pl.rgx), dim3(pl.rblock), 0, s, part,
                       static_cast<float*>(dw), lddw, n, k, slices);
  return vmhost::launch_status("vm_linear_wgrad");
}

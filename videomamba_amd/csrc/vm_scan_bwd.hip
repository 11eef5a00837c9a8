// Selective scan backward (vm_selective_scan_bwd): the gradient of vm_selective_scan_fwd on
// token-major operands with 16 unit-stride states, fp32 or bf16, all arithmetic in fp32.
//
//   delta' = softplus?(delta + bias)        a_t = exp(delta'_t A)
//   h_t = a_t h_{t-1} + delta'_t u_t B_t    y_t = <h_t, C_t> + D u_t    out = y silu(z)
//
//   dy_t = dout_t silu(z_t)                 dz_t = dout_t y_t sig(z_t)(1 + z_t(1 - sig(z_t)))
//   g_t  = C_t dy_t + a_{t+1} g_{t+1}       (g_L = dh_last or 0)
//   dC_t[n] = sum_d h_t dy_t                dB_t[n] = sum_d g_t delta'_t u_t
//   du_t = D dy_t + sum_n g_t delta'_t B_t
//   ddelta'_t = sum_n g_t (A a_t h_{t-1} + u_t B_t)   ddelta_t = ddelta'_t sig(delta_t + bias)
//   dA = sum_{b,t} g_t delta'_t a_t h_{t-1}   dD = sum_{b,t} dy_t u_t   dbias = sum_{b,t} ddelta_t
//   dh0 = a_0 g_0
//
// Structure (ScanBwdPlan, vm_scan_bwd_plan.h): one workgroup of four 64-lane waves per (batch
// row, 64 channels), one lane per channel, each wave owning four of the 16 states, sequential
// in time.
//   Sweep 1 recomputes h over chunks 0 .. nchunks - 2 and writes the state entering every
//   later chunk to the workspace.
//   Sweep 2 walks the chunks backwards: it loads the chunk's operands, recomputes the state
//   entering every step into LDS (h_{t-1} is never reconstructed by dividing by a_t), then
//   runs the g recurrence over the chunk in reverse.  dA accumulates in the owning lane's
//   registers; the per-step cross-channel sums dB | dC are folded over the wave's 64 lanes by
//   a fixed halving tree and stored as per-group partials.  Once per chunk waves 1..3 hand
//   their states' parts of y, du and ddelta' to wave 0 through LDS; wave 0 adds them in wave
//   order, stores du / ddelta / dz and accumulates dD and dbias.
//   scan_bwd_reduce_kernel then adds the group partials (dB, dC) in group order and the
//   batch-row partials (dA, dD, dbias) in batch order.
// No atomics anywhere: every sum has one fixed order, so two launches give equal bits.
// Lanes at or past dim and steps at or past seqlen load nothing outside the operands (they
// re-read the last channel / step and use 0 instead, so they add 0 to every sum) and store
// nothing outside the workspace's padded rows.
//
// Paired form (vm_selective_scan_bidir_bwd, PAIR): the gradient of vm_selective_scan_bidir_fwd
// over batch = 2 split rows in one launch.  A workgroup of a row b >= split (uniform per
// workgroup, so the choice is scalar) takes the backward direction's A / D / bias, its states
// at row b - split, and reads step t's dout at the un-flipped row the forward stored step t's
// output at (PairSel::orow, vm_scan.h); every other operand and gradient stays in flipped
// step order.  The reduce adds the dA / dD / dbias partials of rows [0, split) into the
// forward direction's outputs and those of [split, 2 split) into the backward direction's,
// each in batch-row order: either half's bits are those of a plain launch over its rows.
#include "vm_common.h"
#include "../../include/videomamba_hip_ext.h"
#include "vm_scan.h"
#include "vm_scan_bwd_plan.h"

namespace vm {

struct ScanBwdParams {
  const void* u; const void* delta; const float* A; const void* B; const void* C;
  const float* D; const void* z; const float* dbias; const void* h0;
  const void* dout; const float* dhl;
  void* du; void* ddelta; void* dz; void* dB; void* dC;
  float* dA; float* dD; float* ddbias; float* dh0;
  long long u_sb, u_sl, dl_sb, dl_sl, b_sb, b_sl, c_sb, c_sl, z_sb, z_sl, h0_sb, h0_sd;
  long long do_sb, do_sl, dhl_sb, dhl_sd;
  long long du_sb, du_sl, dd_sb, dd_sl, dz_sb, dz_sl;
  long long dB_sb, dB_sn, dB_sl, dC_sb, dC_sn, dC_sl, dh0_sb, dh0_sd;
  int batch, dim, seqlen, softplus, h0_dtype;
};

// The backward direction of a paired launch: the parameter set, states and parameter
// gradients of batch rows b >= split (state row b - split, the forward direction's dtypes and
// strides) and the constants of their dout row map.  A trailing kernel argument of its own,
// so the plain kernels' argument layout stays what it was.
struct ScanBwdPair {
  int split;
  const float* A; const float* D; const float* dbias; const void* h0; const float* dhl;
  float* dA; float* dD; float* ddbias; float* dh0;
  int ro_c0, ro_s, ro_c1; unsigned ro_m;
};

// Parameter set of batch row b (uniform per workgroup): PairSel's parameters, entry state and
// row map (its last-state slot is unused here) and the state gradients.  PAIR = false folds to
// the plain launch's at compile time.
struct BwdSel {
  PairSel s;
  const float* dhl; float* dh0;
};
template <bool PAIR>
__device__ __forceinline__ BwdSel bwd_sel(const ScanBwdParams& p, const ScanBwdPair& q, int b) {
  if (PAIR && b >= q.split)
    return {{q.A, q.D, q.dbias, q.h0, nullptr, b - q.split, q.ro_c0, q.ro_s, q.ro_c1, q.ro_m},
            q.dhl, q.dh0};
  return {{p.A, p.D, p.dbias, p.h0, nullptr, b, 0, 1, 0, 0u}, p.dhl, p.dh0};
}

__device__ __forceinline__ float lane_value(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Sum of v[j] over the wave's 64 lanes for all 8 j at once: each of three halving stages
// keeps one half of the values and adds the partner lane's copy of it, then three plain
// exchange-adds finish the sum.  Lane l ends with the total of value bitrev3(l & 7).
// 7 + 3 exchanges instead of 8 x 6, in one fixed order.
__device__ __forceinline__ float fold8(float (&v)[2 * kBwdNS], int lane) {
  static_assert(kBwdNS == 4, "fold8 folds 2 x 4 values");
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int k = 4 >> s;
    const bool up = (lane >> s) & 1;
#pragma unroll
    for (int i = 0; i < k; ++i) {
      // read both first: a conditional between two array elements is an lvalue, which the
      // compiler lowers to a lane-indexed walk over the whole array
      const float lo = v[i], hi = v[i + k];
      const float keep = up ? hi : lo;
      const float send = up ? lo : hi;
      v[i] = keep + __shfl_xor(send, 1 << s, 64);
    }
  }
  float r = v[0];
  r += __shfl_xor(r, 8, 64);
  r += __shfl_xor(r, 16, 64);
  r += __shfl_xor(r, 32, 64);
  return r;
}

__device__ __forceinline__ int bitrev3(int l) {
  return ((l & 1) << 2) | (l & 2) | ((l & 4) >> 2);
}

template <typename T, bool HAS_Z, bool PAIR>
__global__ __launch_bounds__(kBwdLanes * kBwdWaves) void scan_bwd_kernel(const ScanBwdParams p,
                                                                         const ScanBwdPlan pl,
                                                                         float* ws,
                                                                         const ScanBwdPair q) {
  constexpr int NS = kBwdNS;  // states per wave
  // the state entering each step of a chunk, [wave][step][state][lane]
  __shared__ float hs_all[kBwdWaves * kBwdT * NS * kBwdLanes];
  // waves 1.. hand wave 0 their parts of y, du and ddelta', [wave - 1][which][step][lane]
  __shared__ float xch[(kBwdWaves - 1) * 3 * kBwdT * kBwdLanes];
  const int lane = threadIdx.x & (kBwdLanes - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = wave * NS;  // this wave's first state
  float* hs = hs_all + wave * (kBwdT * NS * kBwdLanes);
  const int grp = blockIdx.x, b = blockIdx.y;
  const int d = grp * kBwdLanes + lane;
  const bool live = d < p.dim;
  const int L = p.seqlen;
  const int nch = pl.nchunks;
  const BwdSel sel = bwd_sel<PAIR>(p, q, b);
  const PairSel& ps = sel.s;
  const int hb = PAIR ? ps.hb : b;  // the state row of this batch row

  float A1[NS], A2[NS];  // A and A log2(e)
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    A1[n] = live ? ps.A[static_cast<long long>(d) * kBwdN + n0 + n] : 0.0f;
    A2[n] = A1[n] * kLog2e;
  }
  const float Dv = (ps.D && live) ? ps.D[d] : 0.0f;
  const float bias = (ps.dbias && live) ? ps.dbias[d] : 0.0f;
  // Every operand load is unconditional from an address inside the operand: a lane past dim
  // reads channel dim - 1, a step past seqlen reads step seqlen - 1, and the value is then
  // replaced by 0.  (A load under a lane-dependent branch is waited for on the spot, which
  // serialises a chunk's 40 loads; these stay in flight together.)
  const int dc = live ? d : p.dim - 1;
  const T* up = static_cast<const T*>(p.u) + b * p.u_sb + dc;
  const T* dlp = static_cast<const T*>(p.delta) + b * p.dl_sb + dc;
  const T* zp = HAS_Z ? static_cast<const T*>(p.z) + b * p.z_sb + dc : nullptr;
  const T* gop = static_cast<const T*>(p.dout) + b * p.do_sb + dc;
  // lanes 0..15 hold B_t[lane], lanes 16..31 C_t[lane - 16]; lanes 32.. repeat them unread
  const int bl = lane & (kBwdN - 1);
  const bool b_lane = (lane & kBwdN) == 0;
  const T* bcp = b_lane ? static_cast<const T*>(p.B) + b * p.b_sb + bl
                        : static_cast<const T*>(p.C) + b * p.c_sb + bl;
  const long long bc_sl = b_lane ? p.b_sl : p.c_sl;

  auto entry_state = [&](float (&h)[NS]) {
#pragma unroll
    for (int n = 0; n < NS; ++n)
      h[n] = (ps.h0 && live) ? load_dyn(ps.h0, hb * p.h0_sb + d * p.h0_sd + n0 + n, p.h0_dtype)
                             : 0.0f;
  };
  auto step_size = [&](float raw) { return p.softplus ? softplus_fast(raw) : raw; };
  auto ckpt_at = [&](int c) {  // this wave's states entering chunk c >= 1
    return ws + pl.ckpt +
           (((static_cast<size_t>(b) * (nch - 1) + (c - 1)) * pl.groups + grp) * kBwdN + n0) *
               kBwdLanes +
           lane;
  };

  // ---- sweep 1: the state entering chunks 1 .. nch - 1 (whole chunks only)
  {
    float h[NS];
    entry_state(h);
    for (int c = 0; c + 1 < nch; ++c) {
      const int t0 = c * kBwdT;
      float uu[kBwdT], raw[kBwdT], bc[kBwdT];
#pragma unroll
      for (int s = 0; s < kBwdT; ++s) {
        const long long t = t0 + s;
        const float uv = to_f32(up[t * p.u_sl]), dv = to_f32(dlp[t * p.dl_sl]);
        uu[s] = live ? uv : 0.0f;
        raw[s] = live ? dv + bias : 0.0f;
        bc[s] = to_f32(bcp[t * bc_sl]);
      }
#pragma unroll
      for (int s = 0; s < kBwdT; ++s) {
        const float dl = live ? step_size(raw[s]) : 0.0f;
        const float du = dl * uu[s];
#pragma unroll
        for (int n = 0; n < NS; ++n)
          h[n] = fmaf(__builtin_amdgcn_exp2f(dl * A2[n]), h[n], du * lane_value(bc[s], n0 + n));
      }
      float* ck = ckpt_at(c + 1);
#pragma unroll
      for (int n = 0; n < NS; ++n) ck[n * kBwdLanes] = h[n];
    }
  }

  // ---- sweep 2: the chunks in reverse
  float gc[NS];  // a_{t+1} g_{t+1}
  float accA[NS];
  float accD = 0.0f, accB = 0.0f;  // wave 0 only
#pragma unroll
  for (int n = 0; n < NS; ++n) {
    gc[n] = (sel.dhl && live) ? sel.dhl[hb * p.dhl_sb + d * p.dhl_sd + n0 + n] : 0.0f;
    accA[n] = 0.0f;
  }
  T* dup = static_cast<T*>(p.du) + b * p.du_sb + d;
  T* ddp = static_cast<T*>(p.ddelta) + b * p.dd_sb + d;
  T* dzp = HAS_Z ? static_cast<T*>(p.dz) + b * p.dz_sb + d : nullptr;
  float* part = ws + pl.bc + (static_cast<size_t>(b) * pl.groups + grp) * L * (2 * kBwdN);
  // fold8 leaves value j = bitrev3(lane & 7) in the lane: dB state n0 + j for j < NS, dC after
  const int fj = bitrev3(lane & 7);
  const int slot = fj < NS ? n0 + fj : kBwdN + n0 + (fj - NS);

  for (int c = nch - 1; c >= 0; --c) {
    const int t0 = c * kBwdT;
    const int nst = L - t0 < kBwdT ? L - t0 : kBwdT;
    float h[NS];
    if (c == 0) {
      entry_state(h);
    } else {
      const float* ck = ckpt_at(c);
#pragma unroll
      for (int n = 0; n < NS; ++n) h[n] = ck[n * kBwdLanes];
    }
    float uu[kBwdT], raw[kBwdT], dl[kBwdT], zz[kBwdT], go[kBwdT], bc[kBwdT];
#pragma unroll
    for (int s = 0; s < kBwdT; ++s) {
      const long long t = s < nst ? t0 + s : L - 1;
      const bool on = s < nst && live;
      const float uv = to_f32(up[t * p.u_sl]), dv = to_f32(dlp[t * p.dl_sl]);
      // paired: the row the forward stored step t's output at (the clamped step's: a valid row)
      const long long tg = PAIR ? ps.orow(static_cast<int>(t)) : t;
      const float gv = to_f32(gop[tg * p.do_sl]);
      uu[s] = on ? uv : 0.0f;
      raw[s] = on ? dv + bias : 0.0f;
      go[s] = on ? gv : 0.0f;
      zz[s] = 0.0f;
      if (HAS_Z) {
        const float zv = to_f32(zp[t * p.z_sl]);
        zz[s] = on ? zv : 0.0f;
      }
      bc[s] = to_f32(bcp[t * bc_sl]);
    }
    // the state entering every step of the chunk
#pragma unroll
    for (int s = 0; s < kBwdT; ++s) {
      if (s < nst) {
        dl[s] = live ? step_size(raw[s]) : 0.0f;
        const float du = dl[s] * uu[s];
#pragma unroll
        for (int n = 0; n < NS; ++n) {
          hs[(s * NS + n) * kBwdLanes + lane] = h[n];
          h[n] = fmaf(__builtin_amdgcn_exp2f(dl[s] * A2[n]), h[n], du * lane_value(bc[s], n0 + n));
        }
      } else {
        dl[s] = 0.0f;
      }
    }
    float py[kBwdT], pdu[kBwdT], pdd[kBwdT];  // this wave's states' parts of y, du, ddelta'
#pragma unroll
    for (int s = kBwdT - 1; s >= 0; --s) {
      py[s] = pdu[s] = pdd[s] = 0.0f;
      if (s < nst) {
        const long long t = t0 + s;
        const float u = uu[s], dlt = dl[s];
        const float dy = HAS_Z ? go[s] * silu_fast(zz[s]) : go[s];
        const float dlu = dlt * u;
        float y = 0.0f, dusum = 0.0f, ddl = 0.0f;
        float v[2 * NS];
#pragma unroll
        for (int n = 0; n < NS; ++n) {
          const float Bn = lane_value(bc[s], n0 + n), Cn = lane_value(bc[s], kBwdN + n0 + n);
          const float hp = hs[(s * NS + n) * kBwdLanes + lane];
          const float a = __builtin_amdgcn_exp2f(dlt * A2[n]);
          const float hn = fmaf(a, hp, dlu * Bn);
          y = fmaf(hn, Cn, y);
          const float g = fmaf(Cn, dy, gc[n]);
          v[n] = g * dlu;
          v[NS + n] = hn * dy;
          const float gd = g * dlt;
          const float ahp = a * hp;
          dusum = fmaf(gd, Bn, dusum);
          ddl = fmaf(g, fmaf(A1[n], ahp, u * Bn), ddl);
          accA[n] = fmaf(gd, ahp, accA[n]);
          gc[n] = a * g;
        }
        py[s] = y; pdu[s] = dusum; pdd[s] = ddl;
        const float tot = fold8(v, lane);
        if (lane < 2 * NS) part[t * (2 * kBwdN) + slot] = tot;
      }
    }
    // waves 1.. hand their parts to wave 0, which adds them in wave order and stores the
    // chunk's du / ddelta / dz
    if (wave > 0) {
      float* x = xch + (wave - 1) * (3 * kBwdT * kBwdLanes) + lane;
#pragma unroll
      for (int s = 0; s < kBwdT; ++s) {
        x[(0 * kBwdT + s) * kBwdLanes] = py[s];
        x[(1 * kBwdT + s) * kBwdLanes] = pdu[s];
        x[(2 * kBwdT + s) * kBwdLanes] = pdd[s];
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int s = kBwdT - 1; s >= 0; --s) {
        if (s < nst) {
          const long long t = t0 + s;
          float y = py[s], dusum = pdu[s], ddl = pdd[s];
#pragma unroll
          for (int w = 1; w < kBwdWaves; ++w) {
            const float* x = xch + (w - 1) * (3 * kBwdT * kBwdLanes) + lane;
            y += x[(0 * kBwdT + s) * kBwdLanes];
            dusum += x[(1 * kBwdT + s) * kBwdLanes];
            ddl += x[(2 * kBwdT + s) * kBwdLanes];
          }
          const float u = uu[s];
          y = fmaf(Dv, u, y);
          float sz = 1.0f, dsz = 0.0f;
          if (HAS_Z) {
            const float sig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-zz[s] * kLog2e));
            sz = zz[s] * sig;
            dsz = sig * fmaf(zz[s], 1.0f - sig, 1.0f);
          }
          const float dy = go[s] * sz;
          float ddelta = ddl;
          if (p.softplus && raw[s] <= 20.0f)
            ddelta *= __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-raw[s] * kLog2e));
          accB += ddelta;
          accD = fmaf(dy, u, accD);
          if (live) {
            dup[t * p.du_sl] = from_f32<T>(fmaf(Dv, dy, dusum));
            ddp[t * p.dd_sl] = from_f32<T>(ddelta);
            if (HAS_Z) dzp[t * p.dz_sl] = from_f32<T>(go[s] * y * dsz);
          }
        }
      }
    }
    __syncthreads();  // xch is free for the next chunk
  }

  if (sel.dh0 && live) {
#pragma unroll
    for (int n = 0; n < NS; ++n) sel.dh0[hb * p.dh0_sb + d * p.dh0_sd + n0 + n] = gc[n];
  }
  const size_t row = static_cast<size_t>(b) * pl.dpad + d;  // d < dpad: inside the padded rows
#pragma unroll
  for (int n = 0; n < NS; ++n) ws[pl.pa + row * kBwdN + n0 + n] = accA[n];
  if (wave == 0) {
    ws[pl.pd + row] = accD;
    ws[pl.pb + row] = accB;
  }
}

// dB | dC: the group partials of every (batch row, step, state) added in group order; dA, dD,
// dbias: the batch-row partials added in batch order.  One thread per output element.
// PAIR: two sets of dA / dD / dbias, the forward direction's from rows [0, split) and the
// backward direction's from rows [split, batch), each from 0 in batch order.
template <typename T, bool PAIR>
__global__ __launch_bounds__(256) void scan_bwd_reduce_kernel(const ScanBwdParams p,
                                                              const ScanBwdPlan pl,
                                                              const float* ws,
                                                              const ScanBwdPair q) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  const long long L = p.seqlen;
  const long long nbc = static_cast<long long>(p.batch) * L * (2 * kBwdN);
  if (i < nbc) {
    const int j = static_cast<int>(i % (2 * kBwdN));
    const long long t = (i / (2 * kBwdN)) % L;
    const long long b = i / (2 * kBwdN) / L;
    const float* src = ws + pl.bc + (static_cast<size_t>(b) * pl.groups * L + t) * (2 * kBwdN) + j;
    float acc = 0.0f;
    for (int g = 0; g < pl.groups; ++g) acc += src[static_cast<size_t>(g) * L * (2 * kBwdN)];
    if (j < kBwdN)
      static_cast<T*>(p.dB)[b * p.dB_sb + j * p.dB_sn + t * p.dB_sl] = from_f32<T>(acc);
    else
      static_cast<T*>(p.dC)[b * p.dC_sb + (j - kBwdN) * p.dC_sn + t * p.dC_sl] = from_f32<T>(acc);
    return;
  }
  long long k = i - nbc;
  const long long na = static_cast<long long>(p.dim) * kBwdN;
  int b0 = 0, b1 = p.batch;  // the batch rows summed
  float* dA = p.dA;
  float* dD = p.dD;
  float* ddbias = p.ddbias;
  if (PAIR) {
    b1 = q.split;
    if (k >= na + p.dim) {  // the backward direction's set
      k -= na + p.dim;
      b0 = q.split; b1 = p.batch;
      dA = q.dA; dD = q.dD; ddbias = q.ddbias;
    }
  }
  if (k < na) {
    const long long d = k / kBwdN;
    const int n = static_cast<int>(k % kBwdN);
    float acc = 0.0f;
    for (int b = b0; b < b1; ++b)
      acc += ws[pl.pa + (static_cast<size_t>(b) * pl.dpad + d) * kBwdN + n];
    dA[k] = acc;
  } else if (k < na + p.dim) {
    const long long d = k - na;
    float accD = 0.0f, accB = 0.0f;
    for (int b = b0; b < b1; ++b) {
      accD += ws[pl.pd + static_cast<size_t>(b) * pl.dpad + d];
      accB += ws[pl.pb + static_cast<size_t>(b) * pl.dpad + d];
    }
    if (dD) dD[d] = accD;
    if (ddbias) ddbias[d] = accB;
  }
}

template <typename T, bool PAIR>
static void scan_bwd_launch(const ScanBwdParams& p, const ScanBwdPair& q, const ScanBwdPlan& pl,
                            float* ws, hipStream_t s) {
  if (p.batch > 0) {
    const dim3 grid(pl.groups, p.batch);
    if (p.z)
      hipLaunchKernelGGL((scan_bwd_kernel<T, true, PAIR>), grid, dim3(kBwdLanes * kBwdWaves), 0,
                         s, p, pl, ws, q);
    else
      hipLaunchKernelGGL((scan_bwd_kernel<T, false, PAIR>), grid, dim3(kBwdLanes * kBwdWaves), 0,
                         s, p, pl, ws, q);
  }
  const long long outs = static_cast<long long>(p.batch) * p.seqlen * (2 * kBwdN) +
                         static_cast<long long>(p.dim) * (kBwdN + 1) * (PAIR ? 2 : 1);
  hipLaunchKernelGGL((scan_bwd_reduce_kernel<T, PAIR>),
                     dim3(static_cast<unsigned>((outs + 255) / 256)), dim3(256), 0, s, p, pl, ws,
                     q);
}

}  // namespace vm

using namespace vm;

extern "C" long long vm_selective_scan_bwd_workspace_bytes(int batch, int dim, int seqlen,
                                                           int dstate) {
  if (dstate != kBwdN) return 0;
  return static_cast<long long>(plan_scan_bwd(batch, dim, seqlen).ws_bytes);
}

namespace {
// The backward direction's arguments of the paired entry; nullptr for the plain entry.
struct PairBwdArgs {
  int split; const float* A; const float* D; const float* dbias; const void* h0;
  const float* dhl; float* dA; float* dD; float* ddbias; float* dh0; int frame_len;
};
}  // namespace

#define VM_SCAN_BWD_ARGS                                                                        \
  const void *u, long long u_sb, long long u_sd, long long u_sl, const void *delta,             \
      long long dl_sb, long long dl_sd, long long dl_sl, const float *A, const void *B,         \
      long long b_sb, long long b_sn, long long b_sl, const void *C, long long c_sb,            \
      long long c_sn, long long c_sl, const float *D, const void *z, long long z_sb,            \
      long long z_sd, long long z_sl, const float *delta_bias, int delta_softplus,              \
      const void *h0, int h0_dtype, long long h0_sb, long long h0_sd, const void *dout,         \
      long long do_sb, long long do_sd, long long do_sl, const float *dh_last,                  \
      long long dhl_sb, long long dhl_sd, void *du, long long du_sb, long long du_sd,           \
      long long du_sl, void *ddelta, long long dd_sb, long long dd_sd, long long dd_sl,         \
      void *dz, long long dz_sb, long long dz_sd, long long dz_sl, void *dB, long long dB_sb,   \
      long long dB_sn, long long dB_sl, void *dC, long long dC_sb, long long dC_sn,             \
      long long dC_sl, float *dA, float *dD, float *ddelta_bias, float *dh0, long long dh0_sb,  \
      long long dh0_sd, int batch, int dim, int seqlen, int dstate, int dtype
#define VM_SCAN_BWD_PASS                                                                        \
  u, u_sb, u_sd, u_sl, delta, dl_sb, dl_sd, dl_sl, A, B, b_sb, b_sn, b_sl, C, c_sb, c_sn, c_sl, \
      D, z, z_sb, z_sd, z_sl, delta_bias, delta_softplus, h0, h0_dtype, h0_sb, h0_sd, dout,     \
      do_sb, do_sd, do_sl, dh_last, dhl_sb, dhl_sd, du, du_sb, du_sd, du_sl, ddelta, dd_sb,     \
      dd_sd, dd_sl, dz, dz_sb, dz_sd, dz_sl, dB, dB_sb, dB_sn, dB_sl, dC, dC_sb, dC_sn, dC_sl,  \
      dA, dD, ddelta_bias, dh0, dh0_sb, dh0_sd, batch, dim, seqlen, dstate, dtype

// Both entries: every check, then the launch.  `pair` adds the paired entry's checks and
// selects the PAIR kernels.
static int scan_bwd_entry(const char* name, VM_SCAN_BWD_ARGS, const PairBwdArgs* pair,
                          void* workspace, long long workspace_bytes, vm_stream_t stream) {
  if (!u || !delta || !A || !B || !C || !dout || !du || !ddelta || !dB || !dC || !dA ||
      (z != nullptr) != (dz != nullptr) || (D != nullptr) != (dD != nullptr) ||
      (delta_bias != nullptr) != (ddelta_bias != nullptr)) {
    vmhost::set_error("%s: null required pointer (dz / dD / ddelta_bias go with z / D / "
                      "delta_bias)", name);
    return VM_E_INVALID;
  }
  if (pair && (!pair->A || !pair->dA || (pair->D != nullptr) != (pair->dD != nullptr) ||
               (pair->dbias != nullptr) != (pair->ddbias != nullptr))) {
    vmhost::set_error("%s: null required pointer (A_bwd and dA_bwd are required; dD_bwd / "
                      "ddelta_bias_bwd go with D_bwd / delta_bias_bwd)", name);
    return VM_E_INVALID;
  }
  if (batch < 0 || dim < 0 || seqlen < 0 || dstate != kBwdN) {
    vmhost::set_error("%s: bad shape batch=%d dim=%d seqlen=%d dstate=%d (dstate must be %d)",
                      name, batch, dim, seqlen, dstate, kBwdN);
    return VM_E_INVALID;
  }
  if (pair) {
    const int F = pair->frame_len;
    if (pair->split < 0 || 2ll * pair->split != batch) {
      vmhost::set_error("%s: batch=%d must be 2*split (split=%d)", name, batch, pair->split);
      return VM_E_INVALID;
    }
    if (F < 1 || seqlen % F || static_cast<long long>(seqlen) * F >= (1ll << 31)) {
      vmhost::set_error("%s: frame_len=%d must be >= 1 and divide seqlen=%d "
                        "(seqlen * frame_len < 2^31)", name, F, seqlen);
      return VM_E_INVALID;
    }
    if ((D != nullptr) != (pair->D != nullptr) ||
        (delta_bias != nullptr) != (pair->dbias != nullptr) ||
        (h0 != nullptr) != (pair->h0 != nullptr)) {
      vmhost::set_error("%s: D / delta_bias / h0 must be present in both directions or in "
                        "neither", name);
      return VM_E_INVALID;
    }
  }
  if (!vmhost::dtype_ok(dtype) || (h0 && !vmhost::dtype_ok(h0_dtype))) {
    vmhost::set_error("%s: unsupported dtype", name);
    return VM_E_INVALID;
  }
  if (u_sd != 1 || dl_sd != 1 || do_sd != 1 || du_sd != 1 || dd_sd != 1 ||
      (z && (z_sd != 1 || dz_sd != 1)) || b_sn != 1 || c_sn != 1) {
    vmhost::set_error("%s: token-major operands only: u / delta / z / dout and their gradients "
                      "need a unit channel stride, B / C a unit state stride", name);
    return VM_E_INVALID;
  }
  const ScanBwdPlan pl = plan_scan_bwd(batch, dim, seqlen);
  if (pl.ws_bytes > 0 &&
      (!workspace || workspace_bytes < static_cast<long long>(pl.ws_bytes))) {
    vmhost::set_error("%s: workspace of %lld bytes, need %zu "
                      "(vm_selective_scan_bwd_workspace_bytes)", name,
                      workspace ? workspace_bytes : 0ll, pl.ws_bytes);
    return VM_E_INVALID;
  }
  if (dim == 0) return VM_OK;
  ScanBwdParams p{};
  p.u = u; p.delta = delta; p.A = A; p.B = B; p.C = C; p.D = D; p.z = z; p.dbias = delta_bias;
  p.h0 = h0; p.dout = dout; p.dhl = dh_last;
  p.du = du; p.ddelta = ddelta; p.dz = dz; p.dB = dB; p.dC = dC;
  p.dA = dA; p.dD = dD; p.ddbias = ddelta_bias; p.dh0 = dh0;
  p.u_sb = u_sb; p.u_sl = u_sl; p.dl_sb = dl_sb; p.dl_sl = dl_sl; p.b_sb = b_sb; p.b_sl = b_sl;
  p.c_sb = c_sb; p.c_sl = c_sl; p.z_sb = z_sb; p.z_sl = z_sl; p.h0_sb = h0_sb; p.h0_sd = h0_sd;
  p.do_sb = do_sb; p.do_sl = do_sl; p.dhl_sb = dhl_sb; p.dhl_sd = dhl_sd;
  p.du_sb = du_sb; p.du_sl = du_sl; p.dd_sb = dd_sb; p.dd_sl = dd_sl;
  p.dz_sb = dz_sb; p.dz_sl = dz_sl;
  p.dB_sb = dB_sb; p.dB_sn = dB_sn; p.dB_sl = dB_sl;
  p.dC_sb = dC_sb; p.dC_sn = dC_sn; p.dC_sl = dC_sl; p.dh0_sb = dh0_sb; p.dh0_sd = dh0_sd;
  p.batch = batch; p.dim = dim; p.seqlen = seqlen; p.softplus = delta_softplus;
  p.h0_dtype = h0_dtype;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  ScanBwdPair q{};
  if (pair) {
    q.split = pair->split; q.A = pair->A; q.D = pair->D; q.dbias = pair->dbias; q.h0 = pair->h0;
    q.dhl = pair->dhl; q.dA = pair->dA; q.dD = pair->dD; q.ddbias = pair->ddbias;
    q.dh0 = pair->dh0;
    pair_row_map(seqlen, pair->frame_len, q.ro_c0, q.ro_s, q.ro_c1, q.ro_m);
    if (dtype == VM_DTYPE_BF16) scan_bwd_launch<bf16_t, true>(p, q, pl, ws, s);
    else scan_bwd_launch<float, true>(p, q, pl, ws, s);
  } else {
    if (dtype == VM_DTYPE_BF16) scan_bwd_launch<bf16_t, false>(p, q, pl, ws, s);
    else scan_bwd_launch<float, false>(p, q, pl, ws, s);
  }
  return vmhost::launch_status(name);
}

extern "C" int vm_selective_scan_bwd(VM_SCAN_BWD_ARGS, void* workspace,
                                     long long workspace_bytes, vm_stream_t stream) {
  return scan_bwd_entry("vm_selective_scan_bwd", VM_SCAN_BWD_PASS, nullptr, workspace,
                        workspace_bytes, stream);
}

extern "C" int vm_selective_scan_bidir_bwd(VM_SCAN_BWD_ARGS, int split, const float* A_bwd,
                                           const float* D_bwd, const float* delta_bias_bwd,
                                           const void* h0_bwd, const float* dh_last_bwd,
                                           float* dA_bwd, float* dD_bwd, float* ddelta_bias_bwd,
                                           float* dh0_bwd, int frame_len, void* workspace,
                                           long long workspace_bytes, vm_stream_t stream) {
  const PairBwdArgs pair{split, A_bwd, D_bwd, delta_bias_bwd, h0_bwd, dh_last_bwd,
                         dA_bwd, dD_bwd, ddelta_bias_bwd, dh0_bwd, frame_len};
  return scan_bwd_entry("vm_selective_scan_bidir_bwd", VM_SCAN_BWD_PASS, &pair, workspace,
                        workspace_bytes, stream);
}


// Shared declarations of the token-major mixer-middle kernels (vm_conv_proj.hip: one
// workgroup per 64 token rows, all channels; vm_conv_proj_sk.hip: the split-K and fused
// forms used for small batches; vm_inproj_conv.hip: the in_proj epilogue form).  Which form
// runs, and every limit, size and launch geometry, is vm_conv_proj_plan.h's.
#pragma once

#include "vm_common.h"
#include "vm_conv_proj_plan.h"

namespace vm {

// Raw arguments of vm_conv_proj_fwd (token-major rows: element (token, channel) at
// base + token * *_tl + channel; tokens are batch-contiguous, token = b * out_len + t).
struct ConvProjTmArgs {
  const bf16_t* x; long long x_tl;
  const float* cw; const float* cb;
  const void* csi; int csi_dtype; long long csi_sb, csi_sd;
  void* cso; int cso_dtype; long long cso_sb, cso_sd;  // new conv state (nullable)
  const bf16_t* wx; int e, e_pad;
  const bf16_t* wdt; int r, r_pad;   // wdt == nullptr: no dt_proj
  bf16_t* u; long long u_tl;
  bf16_t* xdbl; long long xd_tl;
  bf16_t* dt; long long dt_tl;
  int out_len, batch, dim, seqlen, width;
};

// Kernel argument of the split-K and fused forms
struct SkTmParams {
  ConvProjTmArgs a;
  float* part;  // [nsplit][ntok][ep] fp32 partials of x_dbl, ep = round_up(e, 4)
  int ntok, nsplit, ep;
};

// The token-major entries' arguments as ConvProjTmArgs; dt == NULL drops W_dt (no dt_proj)
inline ConvProjTmArgs conv_proj_tm_args(
    const void* x, long long x_tl, const float* cw, const float* cb,
    const void* csi, int csi_dtype, long long csi_sb, long long csi_sd,
    void* cso, int cso_dtype, long long cso_sb, long long cso_sd,
    const void* wx, int e, int e_pad, const void* wdt, int r, int r_pad,
    void* u, long long u_tl, void* xdbl, long long xd_tl, void* dt, long long dt_tl,
    int out_len, int batch, int dim, int seqlen, int width) {
  ConvProjTmArgs a{};
  a.x = static_cast<const bf16_t*>(x); a.x_tl = x_tl; a.cw = cw; a.cb = cb;
  a.csi = csi; a.csi_dtype = csi_dtype; a.csi_sb = csi_sb; a.csi_sd = csi_sd;
  a.cso = cso; a.cso_dtype = cso_dtype; a.cso_sb = cso_sb; a.cso_sd = cso_sd;
  a.wx = static_cast<const bf16_t*>(wx); a.e = e; a.e_pad = e_pad;
  a.wdt = dt ? static_cast<const bf16_t*>(wdt) : nullptr; a.r = r; a.r_pad = r_pad;
  a.u = static_cast<bf16_t*>(u); a.u_tl = u_tl;
  a.xdbl = static_cast<bf16_t*>(xdbl); a.xd_tl = xd_tl;
  a.dt = static_cast<bf16_t*>(dt); a.dt_tl = dt_tl;
  a.out_len = out_len; a.batch = batch; a.dim = dim; a.seqlen = seqlen; a.width = width;
  return a;
}

// The shape facts of those arguments as the plan's input (the caller adds what the
// arguments do not carry: xz_sb, dt_softplus, the in_proj operands)
inline ConvProjPlanIn conv_proj_plan_in(const ConvProjTmArgs& a, ConvProjEntry entry) {
  ConvProjPlanIn in{};
  in.layout = ConvProjLayout::kTokenMajor;
  in.entry = entry;
  in.batch = a.batch; in.out_len = a.out_len; in.seqlen = a.seqlen; in.dim = a.dim;
  in.e = a.e; in.e_pad = a.e_pad; in.r = a.r; in.r_pad = a.r_pad; in.width = a.width;
  in.want_dt = a.wdt != nullptr;
  in.xz_sl = a.x_tl; in.u_sl = a.u_tl;
  in.has_cs_in = a.csi != nullptr; in.has_cs_out = a.cso != nullptr;
  in.cs_in_bf16 = a.csi_dtype == VM_DTYPE_BF16;
  in.csi_sb = a.csi_sb; in.csi_sd = a.csi_sd;
  return in;
}

inline SkTmParams sk_tm_params(const ConvProjTmArgs& a, const ConvProjPlan& pl, float* part) {
  SkTmParams q{};
  q.a = a;
  q.part = part;
  q.ntok = pl.ntok; q.nsplit = pl.nsplit; q.ep = pl.ep;
  return q;
}

// Launches of vm_conv_proj_sk.hip, geometry and template selectors from the plan
void conv_proj_sk_launch(const SkTmParams& q, const ConvProjPlan& pl, hipStream_t s);
// its second kernel alone (partials -> x_dbl [-> dt]), shared with vm_inproj_conv.hip
void conv_proj_sk_reduce_launch(const SkTmParams& q, const ConvProjPlan& pl, hipStream_t s);
// The fused small-batch form (one launch, no partials; bit-identical to the split-K form)
void conv_proj_fused_launch(const SkTmParams& q, const ConvProjPlan& pl, hipStream_t s);

// Argument checks the three entries word alike
inline int conv_proj_refuse(const char* entry, const char* what) {
  vmhost::set_error("%s: %s", entry, what);
  return VM_E_INVALID;
}
constexpr const char* kConvProjNull = "null required pointer";
constexpr const char* kConvProjAlias = "conv_state_out must not alias conv_state_in";

}  // namespace vm

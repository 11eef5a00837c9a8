// Host-side plan of the mixer middle (conv1d + SiLU -> x_proj -> dt_proj): which of the five
// kernel forms takes a shape, the limits that decide it, the geometry of every launch and
// the workspace it indexes.  Plain C++17, no HIP header: the host queries and the three _fwd
// entries of vm_conv_proj.hip, vm_conv_proj_sk.hip and vm_inproj_conv.hip all read one
// ConvProjPlan, the kernels take their tile sizes, pitches and LDS carve-ups from the
// constants below, and tests/host/conv_proj_plan_check.cpp walks plan_conv_proj() over a
// grid of shapes on the host.  To add or swap a form, change this file and its launch.
#pragma once

#include <cstddef>

#include "vm_gemm_plan.h"

namespace vm {

// ---------------------------------------------------------------- shared constants
// The small-batch forms run for batch <= kSkMaxBatch.  The choice depends on the batch only,
// never on the sequence length, so a sequence run in chunks sees the same arithmetic as the
// full-sequence run (chunked == full bitwise).
constexpr int kSkMaxBatch = 8;
constexpr int kSkMaxEp = 76;   // round_up(R + 2N, 4) the small-batch forms stage per token row
constexpr int kSkCh = 128;     // channels per split: FIXED, so the x_proj reduction order (and
                               // every token's x_dbl bits) never depends on the token count
constexpr int kSkMaxSpl = 16;  // splits the reduce kernels are instantiated for (dim <= 2048)

constexpr int kCPTok = 64;     // wide form: token rows per workgroup
constexpr int kCmTok = 64;     // split-K and channel-major forms: tokens per workgroup
constexpr int kCmPitch = 72;   // LDS row pitch in bf16 (144 B): 16-B aligned rows
constexpr int kCmHalo = 8;     // tokens staged before the tile (>= width - 1, 16-B aligned)
constexpr int kTmPitch = 136;  // LDS row pitch in bf16 (272 B): 128 channels + 16-B pad
// conv-state rows staged per split-K tile: sequences whose first 3 steps touch a 64-token
// tile (out_len >= 8: at most 64 / 8 + 1)
constexpr int kSkMinLen = 8;
constexpr int kSkCsRows = kCmTok / kSkMinLen + 1;

constexpr int kFuTok = 16;      // fused form: token rows per workgroup
constexpr int kFuMaxSpl = 9;    // splits (waves) per workgroup: dim <= 1152
constexpr int kFuUPitch = 136;  // bf16 pitch of a wave's [16 tok][128 ch] u tile
constexpr int kFuXdPitch = 72;  // bf16 pitch of the [16 tok][64] x_dbl[:R] operand
constexpr int kFuXRows = 20;    // x rows staged per wave (tok0 - 3 .. tok0 + 16)
constexpr int kFuMinLen = 24;   // at most one sequence start in tok0 - 2 .. tok0 + 15
constexpr int kFuMaxEpad = 80;  // wider x_proj outputs exceed the 576-thread register budget

constexpr int kIcRow = kGemmRow;  // in_proj form: bytes per staged K row (64 bf16)
constexpr int kIcOut = 112;     // x output rows per tile
constexpr int kIcHalo = 16;     // rows above them computed for the conv
constexpr int kIcPitch = 136;   // bf16 pitch of the LDS x / u tile
constexpr int kIcCsSeq = 3;     // sequences starting in a tile (out_len >= 56)
constexpr int kIcMinLen = 56;
constexpr int kIcStage = (128 + 128) * kIcRow;  // one K-step stage: A and B rows
constexpr int kIcOBytes = 128 * kIcPitch * 2;   // x tile [128][kIcPitch] bf16
constexpr int kIcWBytes = kFuMaxEpad * kIcPitch * 2;  // W_x slice [e_pad <= 80][kIcPitch]
constexpr int kIcCBytes = kIcCsSeq * 3 * 128 * 4;
constexpr int kIcLds = (2 * kIcStage > kIcOBytes + kIcWBytes + kIcCBytes)
                           ? 2 * kIcStage : kIcOBytes + kIcWBytes + kIcCBytes;

// ---------------------------------------------------------------- LDS carve-ups
// Each formula is called by the kernel that carves the LDS up and by the plan that sizes
// the launch.
// Split-K first kernel (dynamic), in bf16 elements: x tile [halo + tok][kTmPitch], u tile
// [tok][kTmPitch], W_x slice [e_pad][kTmPitch]; then the fp32 conv-state taps.
constexpr int sk_u_off() { return (kCmHalo + kCmTok) * kTmPitch; }
constexpr int sk_w_off() { return sk_u_off() + kCmTok * kTmPitch; }
constexpr int sk_c_off(int e_pad) { return sk_w_off() + e_pad * kTmPitch; }
constexpr size_t sk_lds_bytes(int e_pad) {
  return static_cast<size_t>(sk_c_off(e_pad)) * 2 +
         static_cast<size_t>(kSkCsRows) * 3 * kSkCh * sizeof(float);
}
// Fused form (dynamic), in bytes: an area shared in turn by the per-wave u tiles, the split
// partials [split][tok][ep] and the dt tile [tok][dim + 8]; the x_dbl[:R] operand; the
// per-wave staged x rows (256 B each).
constexpr int fu_u_bytes() { return kFuMaxSpl * kFuTok * kFuUPitch * 2; }
constexpr int fu_part_bytes(int nsplit, int ep) { return nsplit * kFuTok * ep * 4; }
constexpr int fu_dt_bytes(int dim) { return kFuTok * (dim + 8) * 2; }
constexpr int fu_area_bytes() {
  return fu_u_bytes() > fu_part_bytes(kFuMaxSpl, kSkMaxEp) ? fu_u_bytes()
                                                           : fu_part_bytes(kFuMaxSpl, kSkMaxEp);
}
constexpr int fu_xrows_off() { return fu_area_bytes() + kFuTok * kFuXdPitch * 2; }
constexpr size_t fu_lds_bytes() {
  return static_cast<size_t>(fu_xrows_off()) + kFuMaxSpl * kFuXRows * 256;
}
static_assert(fu_dt_bytes(kFuMaxSpl * kSkCh) <= fu_part_bytes(kFuMaxSpl, kSkMaxEp),
              "dt tile exceeds the area");
// the split-K and in_proj forms stage 4 waves x 16 partial rows of kSkMaxEp floats in their
// (by then unused) x tile
static_assert(4 * 16 * kSkMaxEp * 4 <= (kCmHalo + kCmTok) * kTmPitch * 2,
              "partial rows exceed the x tile");
// Wide form (dynamic): conv taps [dim][4] and bias [dim] as fp32.
constexpr size_t cp_wide_lds_bytes(int dim) { return static_cast<size_t>(dim) * 5 * sizeof(float); }

constexpr int round_up4(int e) { return (e + 3) / 4 * 4; }
constexpr int sk_splits(int dim) { return (dim + kSkCh - 1) / kSkCh; }

// ---------------------------------------------------------------- the plan
enum class ConvProjLayout { kTokenMajor, kChannelMajor };
// which entry asks: vm_in_proj_conv_proj_* takes the in_proj form or none
enum class ConvProjEntry { kConvProj, kInProjConvProj };

enum class ConvProjForm {
  kNone,          // nothing launches: see ConvProjPlan::why
  kWide,          // conv_proj_kernel: one workgroup per 64 token rows, all channels
  kSplitK,        // conv_xproj_tm_kernel + xdbl_dt_tm_kernel through fp32 partials
  kFused,         // conv_proj_fused_kernel: one launch, bit-identical to split-K
  kInProj,        // inproj_conv_kernel (in_proj epilogue) + a reduce kernel
  kChannelMajor,  // conv_xproj_cm_kernel + xdbl_dt_cm_kernel
};

enum class ConvProjWhy {
  kOk,
  kEmpty,        // batch or out_len <= 0: nothing to do (the fits query reports 1)
  kWideOffsets,  // the wide form's 31-bit buffer offsets do not cover the operands
  kInProjShape,  // outside the in_proj form's shapes, or its 31-bit extents
  kCmShape,      // channel-major: dim % 64 != 0 or a non-positive size
  kSmallXzGap,   // a small form with batch > 1 whose xz rows are not batch-contiguous
};

struct ConvProjPlanIn {
  ConvProjLayout layout;
  ConvProjEntry entry;
  int batch, out_len, seqlen, dim, e, e_pad, r, r_pad, width;
  bool want_dt;      // dt_proj runs here (dt != NULL)
  bool dt_softplus;  // the dt epilogue applies the scan's delta activation
  // row strides, in elements, that the offset limits read (token-major)
  long long xz_sb, xz_sl, u_sl;
  bool has_cs_in, has_cs_out;
  bool cs_in_bf16;          // conv state in is bf16 (else fp32)
  long long csi_sb, csi_sd;
  int k;                    // in_proj's K, or 0
  long long ldh, ldw;       // in_proj operand row strides (0 in the fits query)
};

struct ConvProjLaunch {
  unsigned gx, gy, block;  // gx == 0: not launched
  size_t lds;              // dynamic LDS bytes
};

struct ConvProjPlan {
  ConvProjForm form;
  ConvProjWhy why;
  int ntok, nsplit, ep;    // tokens, 128-channel splits, round_up(e, 4)
  int tiles;               // token tiles of the main launch
  int nxr, nzr;            // in_proj form: x row tiles (kIcOut rows), z row tiles (128 rows)
  int NB, NSPL, NK;        // template selectors: e_pad / 16, splits summed, k / 64
  bool CS32;               // fused form: fp32 conv state in
  ConvProjLaunch main, reduce, state;
  long long ws_query;      // what the form's workspace size query reports
  long long ws_need;       // what the entry asks of the caller
  long long ws_bytes;      // what the launched kernels index
  bool small() const { return form == ConvProjForm::kSplitK || form == ConvProjForm::kFused; }
};

inline ConvProjPlan plan_conv_proj(const ConvProjPlanIn& in) {
  ConvProjPlan pl{};
  pl.form = ConvProjForm::kNone;
  pl.why = ConvProjWhy::kOk;
  const bool sized = in.batch > 0 && in.out_len > 0 && in.dim > 0 && in.e > 0;
  const long long ntok = 1LL * in.batch * in.out_len;
  pl.ntok = static_cast<int>(ntok);
  pl.ep = round_up4(in.e);
  pl.NB = in.e_pad / 16;
  auto tiles_of = [&](int tok) { return static_cast<int>((ntok + tok - 1) / tok); };
  const unsigned dt_blocks = static_cast<unsigned>((in.dim + 127) / 128);

  if (in.layout == ConvProjLayout::kChannelMajor) {
    if (!sized || in.dim % 64 != 0) {
      pl.why = ConvProjWhy::kCmShape;
      return pl;
    }
    pl.form = ConvProjForm::kChannelMajor;
    pl.nsplit = sk_splits(in.dim);
    pl.tiles = tiles_of(kCmTok);
    // the channel-major partials are [split][e][tok] with the unrounded e (the token-major
    // forms round e up to 4 for their float4 rows)
    pl.ws_query = pl.ws_need = pl.ws_bytes =
        static_cast<long long>(pl.nsplit) * in.e * pl.ntok * static_cast<long long>(sizeof(float));
    pl.main = {static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.nsplit), 256, 0};
    pl.reduce = {static_cast<unsigned>(pl.tiles), dt_blocks, 256, 0};
    if (in.has_cs_out)
      pl.state = {static_cast<unsigned>((in.dim + 255) / 256), static_cast<unsigned>(in.batch), 256, 0};
    return pl;
  }

  // token-major partials [split][tok][ep]
  const long long sk_bytes =
      sized ? sk_splits(in.dim) * ntok * pl.ep * static_cast<long long>(sizeof(float)) : 0;
  const unsigned reduce_gy = in.want_dt ? dt_blocks : 1u;

  if (in.entry == ConvProjEntry::kInProjConvProj) {
    pl.ws_query = pl.ws_need = sk_bytes;
    const bool ok =  // inproj_conv_kernel is instantiated for the projection GEMM's K steps
        gemm_k_ok(in.k) && in.batch >= 1 && in.batch <= kSkMaxBatch && in.dim % 128 == 0 &&
        in.dim <= kSkMaxSpl * kSkCh && in.out_len >= kIcMinLen && in.e_pad <= kFuMaxEpad &&
        in.e_pad % 16 == 0 && pl.ep <= kSkMaxEp && (!in.want_dt || in.r_pad <= 64) &&
        in.width >= 1 && in.width <= 4 &&
        // buffer resources over u, hn, the in_proj weight and the partials: under 2^31 bytes
        ntok * in.u_sl * 2 < (1ll << 31) && ntok * in.ldh * 2 < (1ll << 31) &&
        2ll * in.dim * in.ldw * 2 < (1ll << 31) && ntok <= (1 << 30);
    if (!ok) {
      pl.why = ConvProjWhy::kInProjShape;
      return pl;
    }
    pl.form = ConvProjForm::kInProj;
    pl.nsplit = pl.NSPL = in.dim / kSkCh;
    pl.NK = in.k / kGemmBK;
    pl.nxr = tiles_of(kIcOut);
    pl.nzr = tiles_of(128);
    pl.tiles = pl.nxr;
    pl.ws_bytes = sk_bytes;
    pl.main = {static_cast<unsigned>((pl.nxr + pl.nzr) * pl.nsplit), 1, 512, kIcLds};
    if (in.want_dt)  // the split-K form's second kernel
      pl.reduce = {static_cast<unsigned>(tiles_of(kCmTok)), reduce_gy, 256, 0};
    else             // xdbl_reduce_kernel: one thread per (token, 4 columns)
      pl.reduce = {static_cast<unsigned>((ntok * (pl.ep / 4) + 255) / 256), 1, 256, 0};
    return pl;
  }

  // vm_conv_proj_workspace_bytes sees (batch, out_len, dim, e) only, so it answers for every
  // batch <= kSkMaxBatch, whatever the other small-form conditions below say
  if (in.batch <= kSkMaxBatch) pl.ws_query = sk_bytes;
  if (in.batch <= 0 || in.out_len <= 0) {
    pl.why = ConvProjWhy::kEmpty;
    return pl;
  }
  // The small forms admit r_pad <= 80, not 64 (the fused form and the entry's own argument
  // check narrow it where dt is wanted), and read r_pad even when dt is not wanted: a caller
  // without dt passes r_pad == 0.
  const bool small = in.batch <= kSkMaxBatch && !in.dt_softplus && in.dim <= kSkMaxSpl * kSkCh &&
                     pl.ep <= kSkMaxEp && in.r_pad <= 80 && in.out_len >= kSkMinLen;
  if (small) {
    // the small forms address x as one run of ntok rows (x + token * xz_sl); only the wide
    // form reads xz_sb, so a gap between the batches' rows is refused, not misread
    if (in.batch > 1 && in.xz_sb != static_cast<long long>(in.out_len) * in.xz_sl) {
      pl.why = ConvProjWhy::kSmallXzGap;
      return pl;
    }
    pl.nsplit = pl.NSPL = sk_splits(in.dim);
    pl.ws_need = sk_bytes;
    // one fused launch where it applies, else the two split-K launches; the fused form's
    // buffer byte offsets (x and u rows, 3 rows before the first) must fit 31 bits
    const bool fused = in.dim <= kFuMaxSpl * kSkCh && in.out_len >= kFuMinLen &&
                       in.e_pad <= kFuMaxEpad && (!in.want_dt || in.r_pad <= 64) &&
                       (ntok + 3) * in.xz_sl * 2 < (1ll << 31) &&
                       (ntok + 3) * in.u_sl * 2 < (1ll << 31);
    if (fused) {
      pl.form = ConvProjForm::kFused;
      pl.tiles = tiles_of(kFuTok);
      pl.CS32 = in.has_cs_in && !in.cs_in_bf16;
      pl.main = {static_cast<unsigned>(pl.tiles), 1, static_cast<unsigned>(64 * pl.nsplit),
                 fu_lds_bytes()};
    } else {
      pl.form = ConvProjForm::kSplitK;
      pl.tiles = tiles_of(kCmTok);
      pl.ws_bytes = sk_bytes;
      pl.main = {static_cast<unsigned>(pl.tiles), static_cast<unsigned>(pl.nsplit), 256,
                 sk_lds_bytes(in.e_pad)};
      pl.reduce = {static_cast<unsigned>(pl.tiles), reduce_gy, 256, 0};
    }
    return pl;
  }
  // wide: 31-bit buffer offsets over the x rows of the sequences one workgroup's 64 rows
  // touch, the conv state, and the workgroup's u rows
  constexpr long long kOff31 = 0x7fffff00LL;
  const int cs_es = in.has_cs_in && in.cs_in_bf16 ? 2 : 4;
  const bool offsets_ok =
      ((long long)(kCPTok / in.out_len + 1) * in.xz_sb + (long long)in.seqlen * in.xz_sl + in.dim) * 2 <= kOff31 &&
      (!in.has_cs_in ||
       ((long long)(in.batch - 1) * in.csi_sb + (long long)(in.dim - 1) * in.csi_sd + in.width) * cs_es <= kOff31) &&
      (long long)kCPTok * in.u_sl * 2 <= kOff31;
  if (!offsets_ok) {
    pl.why = ConvProjWhy::kWideOffsets;
    return pl;
  }
  pl.form = ConvProjForm::kWide;
  pl.tiles = tiles_of(kCPTok);
  pl.main = {static_cast<unsigned>(pl.tiles), 1, 256, cp_wide_lds_bytes(in.dim)};
  if (in.has_cs_out)
    pl.state = {static_cast<unsigned>((in.dim + 255) / 256), static_cast<unsigned>(in.batch), 256, 0};
  return pl;
}

}  // namespace vm

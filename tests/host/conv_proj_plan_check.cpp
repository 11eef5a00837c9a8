// Stand-alone check of the mixer middle's host plan (videomamba_amd/csrc/vm_conv_proj_plan.h):
// walks plan_conv_proj() over a grid of shapes and exits non-zero unless every plan picks the
// form the rules below give and is self-consistent.  Built and run by tests/test_api_cpu.py
// with -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>
#include <initializer_list>

#include "vm_conv_proj_plan.h"

using namespace vm;

static long g_fail = 0;
static const ConvProjPlanIn* g_in = nullptr;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) {                                                                            \
      if (g_fail++ < 20)                                                                      \
        std::fprintf(stderr,                                                                  \
                     "line %d: %s  [layout=%d entry=%d B=%d Lp=%d L=%d D=%d e=%d ep=%d "      \
                     "rp=%d dt=%d spd=%d cs=%d/%d k=%d]\n",                                   \
                     __LINE__, #cond, (int)g_in->layout, (int)g_in->entry, g_in->batch,       \
                     g_in->out_len, g_in->seqlen, g_in->dim, g_in->e, g_in->e_pad,            \
                     g_in->r_pad, g_in->want_dt, g_in->dt_softplus, g_in->has_cs_in,          \
                     g_in->cs_in_bf16, g_in->k);                                              \
    }                                                                                         \
  } while (0)

constexpr size_t kLdsPerCu = 160 * 1024;  // MI355X: 160 KB of LDS per CU
constexpr long long k2G = 1ll << 31;

// grid x block x tile covers the tokens, with no idle tile
static void covers(const ConvProjPlan& pl, int tile) {
  CHECK(static_cast<long long>(pl.tiles) * tile >= pl.ntok);
  CHECK(static_cast<long long>(pl.tiles - 1) * tile < pl.ntok);
}

static void check_token_major(const ConvProjPlanIn& in, const ConvProjPlan& pl, long (&seen)[6]) {
  const long long ntok = 1ll * in.batch * in.out_len;
  const int ep = (in.e + 3) / 4 * 4;
  const long long sk_bytes = (in.dim + 127) / 128 * ntok * ep * 4;
  // ---- the form, from the rules written out
  const bool small = in.batch <= 8 && !in.dt_softplus && in.dim <= 2048 && ep <= 76 &&
                     in.r_pad <= 80 && in.out_len >= 8;
  const bool fused = small && in.dim <= 1152 && in.out_len >= 24 && in.e_pad <= 80 &&
                     (!in.want_dt || in.r_pad <= 64) && (ntok + 3) * in.xz_sl * 2 < k2G &&
                     (ntok + 3) * in.u_sl * 2 < k2G;
  const int cs_es = in.has_cs_in && in.cs_in_bf16 ? 2 : 4;
  const bool wide_ok =
      ((64 / in.out_len + 1) * in.xz_sb + in.seqlen * in.xz_sl + in.dim) * 2 <= 0x7fffff00ll &&
      (!in.has_cs_in ||
       ((in.batch - 1) * in.csi_sb + (in.dim - 1) * in.csi_sd + in.width) * cs_es <= 0x7fffff00ll) &&
      64 * in.u_sl * 2 <= 0x7fffff00ll;
  // the small forms read x as one run of ntok rows: a gap between the batches' xz rows
  // (which only the wide form honours) is refused
  const bool gap = small && in.batch > 1 && in.xz_sb != in.out_len * in.xz_sl;
  const ConvProjForm want = gap ? ConvProjForm::kNone
                            : fused ? ConvProjForm::kFused
                            : small ? ConvProjForm::kSplitK
                            : wide_ok ? ConvProjForm::kWide : ConvProjForm::kNone;
  CHECK(pl.form == want);
  CHECK((pl.why == ConvProjWhy::kOk) == (pl.form != ConvProjForm::kNone));
  if (pl.form == ConvProjForm::kNone)
    CHECK(pl.why == (gap ? ConvProjWhy::kSmallXzGap : ConvProjWhy::kWideOffsets));
  ++seen[static_cast<int>(pl.form)];
  // ---- the size query answers for every batch <= 8, the entry asks the small forms only
  CHECK(pl.ws_query == (in.batch <= 8 ? sk_bytes : 0));
  CHECK(pl.ws_need == (small && !gap ? sk_bytes : 0));
  if (pl.form == ConvProjForm::kNone) return;
  CHECK(pl.ntok == ntok && pl.ep == ep && pl.NB == in.e_pad / 16);
  CHECK(pl.main.lds <= kLdsPerCu && pl.reduce.lds == 0 && pl.state.lds == 0);
  CHECK(pl.main.gx >= 1 && pl.main.block >= 64 && pl.main.block <= 1024);
  if (pl.form == ConvProjForm::kWide) {
    CHECK(pl.NB >= 1 && pl.NB <= 8);
    covers(pl, kCPTok);
    CHECK(pl.main.gx == static_cast<unsigned>(pl.tiles) && pl.main.block == 256);
    CHECK(pl.main.lds == static_cast<size_t>(in.dim) * 20);
    CHECK(pl.ws_bytes == 0 && pl.reduce.gx == 0);
    CHECK((pl.state.gx != 0) == in.has_cs_out);
    if (pl.state.gx) CHECK(pl.state.gx * 256ll >= in.dim && pl.state.gy == (unsigned)in.batch);
    // buffer resources: a workgroup's u rows, the conv state
    CHECK(64 * in.u_sl * 2 < k2G);
    if (in.has_cs_in)
      CHECK(((in.batch - 1) * in.csi_sb + (in.dim - 1) * in.csi_sd + in.width) * cs_es < k2G);
    return;
  }
  // the small forms
  CHECK(pl.nsplit == (in.dim + 127) / 128 && pl.NSPL == pl.nsplit);
  CHECK(pl.NSPL >= 1 && pl.NSPL <= 16 && pl.nsplit * kSkCh >= in.dim);
  CHECK(pl.state.gx == 0);  // both write the conv state from their main kernel
  if (pl.form == ConvProjForm::kSplitK) {
    CHECK(pl.NB >= 1 && pl.NB <= 8);
    covers(pl, kCmTok);
    CHECK(pl.main.gx == (unsigned)pl.tiles && pl.main.gy == (unsigned)pl.nsplit && pl.main.block == 256);
    CHECK(pl.main.lds == static_cast<size_t>(72 + 64 + in.e_pad) * 136 * 2 + 9 * 3 * 128 * 4);
    CHECK(pl.reduce.gx == (unsigned)pl.tiles && pl.reduce.block == 256);
    CHECK(pl.reduce.gy == (in.want_dt ? (unsigned)((in.dim + 127) / 128) : 1u));
    // the largest index either kernel forms: nsplit x ntok x ep floats
    CHECK(pl.ws_bytes >= 4ll * pl.nsplit * pl.ntok * pl.ep && pl.ws_bytes <= pl.ws_need);
  } else {
    CHECK(pl.form == ConvProjForm::kFused);
    CHECK(pl.NB >= 1 && pl.NB <= 5 && pl.NSPL <= kFuMaxSpl);
    covers(pl, kFuTok);
    CHECK(pl.main.gx == (unsigned)pl.tiles && pl.main.gy == 1 && pl.main.block == 64u * pl.nsplit);
    CHECK(pl.reduce.gx == 0 && pl.ws_bytes == 0);
    CHECK(pl.CS32 == (in.has_cs_in && !in.cs_in_bf16));
    // its shared area holds this plan's partials and dt tile; the whole carve-up fits
    CHECK(fu_part_bytes(pl.nsplit, pl.ep) <= fu_area_bytes());
    CHECK(fu_dt_bytes(in.dim) <= fu_area_bytes());
    CHECK(pl.main.lds == static_cast<size_t>(fu_area_bytes()) + 16 * 72 * 2 + 9 * 20 * 256);
    // buffer resources over all of x and u
    CHECK(ntok * in.xz_sl * 2 < k2G && ntok * in.u_sl * 2 < k2G);
    CHECK(1ll * in.e_pad * in.dim * 2 < k2G);
  }
}

static void check_in_proj(const ConvProjPlanIn& in, const ConvProjPlan& pl, long (&seen)[6]) {
  const long long ntok = 1ll * in.batch * in.out_len;
  const int ep = (in.e + 3) / 4 * 4;
  const bool sized = in.batch > 0 && in.out_len > 0 && in.dim > 0 && in.e > 0;
  const long long sk_bytes = sized ? (in.dim + 127) / 128 * ntok * ep * 4 : 0;
  const int k = in.k;
  const bool k_ok = k == 192 || k == 384 || k == 576 || k == 768 || k == 1152 || k == 1536;
  const bool want = k_ok && in.batch >= 1 && in.batch <= 8 && in.dim % 128 == 0 && in.dim <= 2048 &&
                    in.out_len >= 56 && in.e_pad <= 80 && in.e_pad % 16 == 0 && ep <= 76 &&
                    (!in.want_dt || in.r_pad <= 64) && in.width >= 1 && in.width <= 4 &&
                    ntok * in.u_sl * 2 < k2G && ntok * in.ldh * 2 < k2G &&
                    2ll * in.dim * in.ldw * 2 < k2G && ntok <= (1 << 30);
  CHECK((pl.form == ConvProjForm::kInProj) == want);
  CHECK(want || (pl.form == ConvProjForm::kNone && pl.why == ConvProjWhy::kInProjShape));
  CHECK(pl.ws_query == sk_bytes && pl.ws_need == sk_bytes);
  ++seen[static_cast<int>(pl.form)];
  if (!want || in.dim <= 0) return;
  CHECK(pl.ntok == ntok && pl.ep == ep);
  CHECK(pl.NB == in.e_pad / 16 && pl.NB >= 1 && pl.NB <= 5);
  CHECK(pl.NK * 64 == k && pl.nsplit * kSkCh == in.dim && pl.NSPL == pl.nsplit && pl.NSPL <= 16);
  CHECK(1ll * pl.nxr * kIcOut >= ntok && 1ll * (pl.nxr - 1) * kIcOut < ntok);
  CHECK(1ll * pl.nzr * 128 >= ntok && 1ll * (pl.nzr - 1) * 128 < ntok);
  CHECK(pl.main.gx == (unsigned)((pl.nxr + pl.nzr) * pl.nsplit) && pl.main.block == 512);
  CHECK(pl.main.lds == kIcLds && pl.main.lds <= kLdsPerCu / 2);  // two workgroups per CU
  CHECK(kIcLds >= 2 * kIcStage && kIcLds >= kIcOBytes + kIcWBytes + kIcCBytes);
  CHECK(in.e_pad * kIcPitch * 2 <= kIcWBytes);
  if (in.want_dt) {
    CHECK(pl.reduce.gx * 64ll >= ntok && pl.reduce.gy == (unsigned)(in.dim / 128));
  } else {
    CHECK(pl.reduce.gx * 256ll >= ntok * (ep / 4) && (pl.reduce.gx - 1) * 256ll < ntok * (ep / 4));
    CHECK(pl.reduce.gy == 1);
  }
  CHECK(pl.reduce.block == 256 && pl.state.gx == 0);
  CHECK(pl.ws_bytes >= 4ll * pl.nsplit * pl.ntok * pl.ep && pl.ws_bytes <= pl.ws_need);
  // buffer resources over hn, the in_proj weight, u and the partials
  CHECK(ntok * in.ldh * 2 < k2G && 4ll * in.dim * in.ldw < k2G && ntok * in.u_sl * 2 < k2G);
  CHECK(pl.ws_bytes < k2G);
}

static void check_channel_major(const ConvProjPlanIn& in, const ConvProjPlan& pl, long (&seen)[6]) {
  const bool want = in.batch > 0 && in.out_len > 0 && in.dim > 0 && in.dim % 64 == 0 && in.e > 0;
  CHECK((pl.form == ConvProjForm::kChannelMajor) == want);
  CHECK(want || (pl.form == ConvProjForm::kNone && pl.why == ConvProjWhy::kCmShape));
  ++seen[static_cast<int>(pl.form)];
  if (!want) {
    CHECK(pl.ws_query == 0);
    return;
  }
  const long long ntok = 1ll * in.batch * in.out_len;
  CHECK(pl.ntok == ntok && pl.nsplit == (in.dim + 127) / 128 && pl.nsplit * 128 >= in.dim);
  CHECK(pl.NB == in.e_pad / 16);
  covers(pl, kCmTok);
  // partials [split][e][tok], e not rounded
  CHECK(pl.ws_bytes == 4ll * pl.nsplit * in.e * ntok);
  CHECK(pl.ws_query == pl.ws_bytes && pl.ws_need == pl.ws_bytes);
  CHECK(pl.main.gx == (unsigned)pl.tiles && pl.main.gy == (unsigned)pl.nsplit);
  CHECK(pl.reduce.gx == (unsigned)pl.tiles && pl.reduce.gy * 128ll >= in.dim);
  CHECK(pl.main.block == 256 && pl.reduce.block == 256 && pl.main.lds == 0 && pl.reduce.lds == 0);
  CHECK((pl.state.gx != 0) == in.has_cs_out);
}

int main() {
  const int Bs[] = {1, 2, 8, 9, 64};
  const int Lps[] = {8, 22, 24, 54, 56, 200, 3144, 300000};
  const int Ds[] = {64, 192, 1152, 1280, 2048, 2112, 8192};
  const int Es[][2] = {{12, 16}, {36, 48}, {68, 80}, {76, 80}, {78, 80}, {84, 96}, {100, 128}};
  const int Rps[] = {0, 32, 64, 80, 96};  // 80: the small forms admit it (see the plan)
  const int Ks[] = {0, 192, 576, 1536, 1024, 200};
  long plans = 0, seen[6] = {0, 0, 0, 0, 0, 0};
  for (int B : Bs) for (int Lp : Lps) for (int D : Ds) for (auto& E : Es) for (int rp : Rps)
  for (int flags = 0; flags < 16; ++flags) {
    ConvProjPlanIn in{};
    in.batch = B; in.out_len = Lp; in.seqlen = Lp > 100 ? Lp - 7 : Lp; in.dim = D;
    in.e = E[0]; in.e_pad = E[1]; in.r = rp ? rp / 2 + 2 : 4; in.r_pad = rp; in.width = 4;
    in.want_dt = flags & 1; in.dt_softplus = flags & 2;
    in.has_cs_in = in.has_cs_out = flags & 4; in.cs_in_bf16 = flags & 8;
    in.xz_sb = 2ll * D * Lp; in.xz_sl = 2 * D; in.u_sl = D;
    in.csi_sb = 4ll * D; in.csi_sd = 4;
    g_in = &in;
    // ---- vm_conv_proj_*
    in.layout = ConvProjLayout::kTokenMajor;
    in.entry = ConvProjEntry::kConvProj;
    check_token_major(in, plan_conv_proj(in), seen);
    ++plans;
    if (flags == 0 || flags == 7) {  // the same shape with 8 rows between the batches' xz
      in.xz_sb += 8 * in.xz_sl;
      check_token_major(in, plan_conv_proj(in), seen);
      ++plans;
      in.xz_sb -= 8 * in.xz_sl;
    }
    // ---- vm_conv_proj_cm_*
    in.layout = ConvProjLayout::kChannelMajor;
    if (flags < 8) {
      check_channel_major(in, plan_conv_proj(in), seen);
      ++plans;
    }
    // ---- vm_in_proj_conv_proj_*
    in.layout = ConvProjLayout::kTokenMajor;
    in.entry = ConvProjEntry::kInProjConvProj;
    if (!(flags & 2))
      for (int k : Ks) for (int w : {4, 2, 0, 5}) {
        in.k = k; in.ldh = in.ldw = k; in.width = w;
        check_in_proj(in, plan_conv_proj(in), seen);
        ++plans;
      }
  }
  // shapes no entry accepts still plan without a fault: empty and negative sizes
  for (int B : {-1, 0, 1}) for (int Lp : {-8, 0, 8}) for (int D : {-128, 0, 100, 128}) for (int e : {-2, 0, 68})
  for (int layout = 0; layout < 3; ++layout) {
    ConvProjPlanIn in{};
    in.layout = layout == 2 ? ConvProjLayout::kChannelMajor : ConvProjLayout::kTokenMajor;
    in.entry = layout == 1 ? ConvProjEntry::kInProjConvProj : ConvProjEntry::kConvProj;
    in.batch = B; in.out_len = Lp; in.seqlen = Lp; in.dim = D; in.e = e; in.e_pad = 80; in.width = 4;
    in.k = 576; in.ldh = in.ldw = 576; in.u_sl = D;
    g_in = &in;
    const ConvProjPlan pl = plan_conv_proj(in);
    ++plans;
    if (B <= 0 || Lp <= 0) {
      CHECK(pl.form == ConvProjForm::kNone && pl.ws_query == 0);
      if (layout == 0) CHECK(pl.why == ConvProjWhy::kEmpty);
    }
    if (layout == 2) check_channel_major(in, pl, seen);
    if (layout == 1) check_in_proj(in, pl, seen);
  }
  // the walk reached every form
  for (int f = 0; f < 6; ++f) {
    if (!seen[f]) {
      std::fprintf(stderr, "form %d never planned\n", f);
      ++g_fail;
    }
  }
  std::printf("%ld plans: none %ld wide %ld split-K %ld fused %ld in_proj %ld channel-major %ld, "
              "%ld failures\n", plans, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5], g_fail);
  return g_fail ? 1 : 0;
}

// Stand-alone query of the mixer middle's host plan (videomamba_amd/csrc/vm_conv_proj_plan.h):
// reads one case per line on stdin, the ConvProjPlanIn fields in the order of
// tests/mixer_mid_matrix.py::Case.plan_line, and prints the name of plan_conv_proj().form
// for each.  Built and run by tests/test_mixer_mid_matrix_cpu.py with
// -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>

#include "vm_conv_proj_plan.h"

using namespace vm;

static const char* form_name(ConvProjForm f) {
  switch (f) {
    case ConvProjForm::kNone: return "none";
    case ConvProjForm::kWide: return "wide";
    case ConvProjForm::kSplitK: return "split_k";
    case ConvProjForm::kFused: return "fused";
    case ConvProjForm::kInProj: return "in_proj";
    case ConvProjForm::kChannelMajor: return "channel_major";
  }
  return "?";
}

int main() {
  long long v[24];
  for (;;) {
    int got = 0;
    while (got < 24 && std::scanf("%lld", &v[got]) == 1) ++got;
    if (got == 0) break;
    if (got != 24) {
      std::fprintf(stderr, "a case needs 24 fields, got %d\n", got);
      return 2;
    }
    ConvProjPlanIn in{};
    in.layout = v[0] ? ConvProjLayout::kChannelMajor : ConvProjLayout::kTokenMajor;
    in.entry = v[1] ? ConvProjEntry::kInProjConvProj : ConvProjEntry::kConvProj;
    in.batch = static_cast<int>(v[2]); in.out_len = static_cast<int>(v[3]);
    in.seqlen = static_cast<int>(v[4]); in.dim = static_cast<int>(v[5]);
    in.e = static_cast<int>(v[6]); in.e_pad = static_cast<int>(v[7]);
    in.r = static_cast<int>(v[8]); in.r_pad = static_cast<int>(v[9]);
    in.width = static_cast<int>(v[10]);
    in.want_dt = v[11] != 0; in.dt_softplus = v[12] != 0;
    in.xz_sb = v[13]; in.xz_sl = v[14]; in.u_sl = v[15];
    in.has_cs_in = v[16] != 0; in.has_cs_out = v[17] != 0; in.cs_in_bf16 = v[18] != 0;
    in.csi_sb = v[19]; in.csi_sd = v[20];
    in.k = static_cast<int>(v[21]); in.ldh = v[22]; in.ldw = v[23];
    const ConvProjPlan pl = plan_conv_proj(in);
    std::printf("%s %d\n", form_name(pl.form), static_cast<int>(pl.why));
  }
  return 0;
}

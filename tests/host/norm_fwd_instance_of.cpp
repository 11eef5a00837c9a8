// Stand-alone query of the norm forward's host plans (videomamba_amd/csrc/vm_norm_plan.h):
// reads one case per line on stdin, a kind and its fields in the order of
// tests/norm_fwd_matrix.py::NormCase.plan_line (kind 1, 11 fields) and PoolCase.plan_line
// (kind 2, 15 fields), and prints the instance plan_add_norm() / plan_norm_pool() names:
//   fast CPL RES RO WT | vec CPL | scalar VPL        and        fast CPL SLICES | generic CPL SLICES
// Kind 0 (no fields) prints kSmallStoreRows and kPoolRB.  A refused case prints "refused WHY".
// Built and run by tests/test_norm_fwd_matrix_cpu.py with -fsanitize=address,undefined; needs
// no GPU and no HIP.
#include <cstdio>

#include "vm_norm_plan.h"

using namespace vm;

static bool read(long long* v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::scanf("%lld", &v[i]) != 1) return false;
  return true;
}

int main() {
  long long kind, v[15];
  while (std::scanf("%lld", &kind) == 1) {
    if (kind == 0) {
      std::printf("consts %lld %d\n", kSmallStoreRows, kPoolRB);
    } else if (kind == 1 && read(v, 11)) {
      AddNormPlanIn in{};
      in.rows = v[0]; in.cols = static_cast<int>(v[1]); in.is_rms = v[2] != 0;
      in.has_bias = v[3] != 0;
      in.x_dtype = static_cast<int>(v[4]); in.out_dtype = static_cast<int>(v[5]);
      in.has_res = v[6] != 0; in.res_dtype = static_cast<int>(v[7]);
      in.has_ro = v[8] != 0; in.ro_dtype = static_cast<int>(v[9]);
      in.x_al = v[10] != 0;
      in.has_x = in.has_weight = in.has_out = true;
      in.res_al = in.w_al = in.out_al = in.ro_al = true;
      const AddNormPlan pl = plan_add_norm(in);
      if (pl.why != NormWhy::kOk)
        std::printf("refused %d\n", static_cast<int>(pl.why));
      else if (pl.family == NormFamily::kFast)
        std::printf("fast %d %d %d %d\n", pl.cpl, pl.res, pl.ro, pl.write_through);
      else
        std::printf("%s %d\n", pl.family == NormFamily::kVec ? "vec" : "scalar", pl.cpl);
    } else if (kind == 2 && read(v, 15)) {
      NormPoolPlanIn in{};
      in.batch = static_cast<int>(v[0]); in.rows = static_cast<int>(v[1]);
      in.cols = static_cast<int>(v[2]); in.head = static_cast<int>(v[3]);
      in.groups = static_cast<int>(v[4]); in.group_rows = static_cast<int>(v[5]);
      in.max_group_rows = static_cast<int>(v[6]); in.has_bounds = v[7] != 0;
      in.x_dtype = static_cast<int>(v[8]); in.out_dtype = static_cast<int>(v[9]);
      in.has_res = v[10] != 0; in.res_dtype = static_cast<int>(v[11]);
      in.rev_frame = static_cast<int>(v[12]);
      in.in_bstride = v[13]; in.out_bstride = v[14];
      in.has_x = in.has_weight = in.has_out = true;
      in.x_al = in.res_al = in.w_al = in.out_al = true;
      const NormPoolPlan pl = plan_norm_pool(in);
      if (pl.why != NormWhy::kOk)
        std::printf("refused %d\n", static_cast<int>(pl.why));
      else
        std::printf("%s %d %d\n", pl.family == NormFamily::kFast ? "fast" : "generic", pl.cpl,
                    pl.slices);
    } else {
      std::fprintf(stderr, "bad case line (kind %lld)\n", kind);
      return 2;
    }
  }
  return 0;
}

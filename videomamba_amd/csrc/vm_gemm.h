// What vm_gemm.hip and vm_gemm_tile.hip share on the host: the operands of one projection
// GEMM call and the launchers that take them with the plan (vm_gemm_plan.h).
#pragma once

#include "vm_common.h"
#include "vm_gemm_plan.h"

namespace vm {

struct GemmArgs {
  const bf16_t* x; long long ldx;  // (m, k)
  const bf16_t* w; long long ldw;  // (n, k)
  const float* bias;               // (n) or null
  bf16_t* out; long long ldo;      // (m, n)
  int m, n, k;
  // vm_linear_add_norm_fwd: res += out (fp32, in place); hn = bf16(rmsnorm(res) * nw)
  float* res; long long ldr;
  const float* nw;
  bf16_t* hn; long long ldh;
  float eps;
  unsigned* cnt;
};

// A launcher fills its kernel's parameter struct and picks the template instance the plan
// names.  A plan without an instance is a bug (tests/host/gemm_plan_check.cpp walks the
// selectors): it launches nothing, sets the error and returns VM_E_INVALID.
int linear_dma_launch(const GemmArgs& a, const GemmPlan& pl, hipStream_t s);  // kDma*
int gemm_tile_launch(const GemmArgs& a, const GemmPlan& pl, hipStream_t s);   // kTile*
int gemm_no_instance(const char* kernel, const GemmPlan& pl);

}  // namespace vm

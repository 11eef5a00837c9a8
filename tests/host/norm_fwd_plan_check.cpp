// Stand-alone check of the norm forward's host plans (videomamba_amd/csrc/vm_norm_plan.h):
// walks plan_add_norm(), plan_norm_pool() and plan_pool_finish() over grids of shapes, dtypes,
// pointer presence and alignment, and exits non-zero unless
//   - cpl 256 >= cols (vpl 64 >= cols) with cpl / vpl the smallest of the family's set, the fast
//     families are chosen exactly when their documented conditions hold, and write-through is
//     res && ro && rows <= kSmallStoreRows;
//   - the grids cover every row, and the pool grid's x extent is max(slices, ceil(head / 16));
//   - the part regions lie back to back from 0 and end exactly at workspace_bytes for every
//     (b, g, s), max_group_rows == 0 included, and the shape-only query equals the plan;
//   - refusals come in the documented order, and the 2^31 switch of the pool's fast family
//     flips at the exact row count.
// Built and run by tests/test_norm_fwd_matrix_cpu.py with -fsanitize=address,undefined; needs
// no GPU and no HIP.
#include <cstdio>
#include <initializer_list>

#include "vm_norm_plan.h"

using namespace vm;

static long g_fail = 0;
static const char* g_what = "";
static long long g_a, g_b, g_c, g_d;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (g_fail++ < 20)                                                                 \
        std::fprintf(stderr, "line %d: %s  [%s %lld %lld %lld %lld]\n", __LINE__, #cond, \
                     g_what, g_a, g_b, g_c, g_d);                                        \
    }                                                                                    \
  } while (0)

static bool in_set(int v, const int (&set)[4]) {
  return v == set[0] || v == set[1] || v == set[2] || v == set[3];
}
// the smallest member of an ascending set that is >= need (its last member past that)
static int smallest(int need, const int (&set)[4]) {
  for (int v : set)
    if (v >= need) return v;
  return set[3];
}
static const int kFastSet[4] = {1, 2, 3, 4}, kVecSet[4] = {1, 2, 4, 8}, kScalarSet[4] = {4, 8, 16, 32};

static long walk_add_norm() {
  g_what = "add_norm rows cols dt bits";
  const long long Rs[] = {0, 1, 3, 4, 5, 32768, 32769, 5000000000LL};
  const int Cs[] = {0, 1, 4, 63, 256, 260, 1024, 1028, 2047, 2048, 2049};
  const int Ds[] = {0, 1, 2, -1};  // fp32, bf16 and two codes that are neither
  long plans = 0;
  for (long long R : Rs) for (int C : Cs)
    for (int dt = 0; dt < 256; ++dt)      // x, res, out, ro: four codes each
      for (int bits = 0; bits < 512; ++bits) {
        // every dtype combination with the pointers present and aligned or not; the
        // presence / alignment bits in full at the all-valid dtype combinations
        const int dx = Ds[dt & 3], dr = Ds[(dt >> 2) & 3], dout = Ds[(dt >> 4) & 3],
                  dro = Ds[(dt >> 6) & 3];
        const bool all_valid = (dt & 0xAA) == 0;
        if (!all_valid && bits != 0 && bits != 0x1f && bits != 0x20 && bits != 0x180) continue;
        g_a = R; g_b = C; g_c = dt; g_d = bits;
        AddNormPlanIn in{};
        in.rows = R; in.cols = C;
        in.x_dtype = dx; in.res_dtype = dr; in.out_dtype = dout; in.ro_dtype = dro;
        // bits 0-4: misaligned x, res, w, out, ro; 5: LayerNorm; 6: bias; 7: no residual;
        // 8: no residual_out
        in.x_al = !(bits & 1); in.res_al = !(bits & 2); in.w_al = !(bits & 4);
        in.out_al = !(bits & 8); in.ro_al = !(bits & 16);
        in.is_rms = !(bits & 32); in.has_bias = bits & 64;
        in.has_res = !(bits & 128); in.has_ro = !(bits & 256);
        in.has_x = in.has_weight = in.has_out = true;
        const AddNormPlan pl = plan_add_norm(in);
        ++plans;
        const bool bad_dtype = (dx != 0 && dx != 1) || (dout != 0 && dout != 1) ||
                               (in.has_res && dr != 0 && dr != 1) ||
                               (in.has_ro && dro != 0 && dro != 1);
        const bool bad = C < 1 || C > 2048 || bad_dtype;
        CHECK((pl.why == NormWhy::kShape) == bad);
        CHECK(pl.why == NormWhy::kOk || pl.why == NormWhy::kShape);
        if (pl.why != NormWhy::kOk) continue;
        CHECK(pl.empty == (R == 0));
        CHECK(pl.block == 256 && 4ll * pl.grid >= R && 4ll * pl.grid < R + 4);
        const bool vec = C % 4 == 0 && in.x_al && in.out_al && in.w_al &&
                         (!in.has_res || in.res_al) && (!in.has_ro || in.ro_al);
        const bool fast = vec && in.is_rms && !in.has_bias && dx == 1 && dout == 1 &&
                          (!in.has_res || dr == 0) && (!in.has_ro || dro == 0) && C <= 1024;
        CHECK((pl.family == NormFamily::kFast) == fast);
        CHECK((pl.family == NormFamily::kVec) == (vec && !fast));
        CHECK((pl.family == NormFamily::kScalar) == !vec);
        if (pl.family == NormFamily::kScalar) {
          CHECK(in_set(pl.cpl, kScalarSet) && pl.cpl * 64 >= C);
          CHECK(pl.cpl == smallest((C + 63) / 64, kScalarSet));
        } else {
          const int (&set)[4] = fast ? kFastSet : kVecSet;
          CHECK(in_set(pl.cpl, set) && pl.cpl * 256 >= C);
          CHECK(pl.cpl == smallest((C + 255) / 256, set));
        }
        if (fast) {
          CHECK(pl.res == in.has_res && pl.ro == in.has_ro);
          CHECK(pl.write_through == (pl.res && pl.ro && R <= kSmallStoreRows));
        } else {
          CHECK(!pl.write_through);
        }
      }
  // refusals: a null pointer before a bad shape, a bad shape before an empty call
  g_what = "add_norm refusals";
  AddNormPlanIn in{};
  in.rows = -1; in.cols = 0; in.x_dtype = 9;
  in.has_x = in.has_weight = in.has_out = true;
  CHECK(plan_add_norm(in).why == NormWhy::kShape);
  for (int miss = 0; miss < 3; ++miss) {
    AddNormPlanIn n = in;
    (miss == 0 ? n.has_x : miss == 1 ? n.has_weight : n.has_out) = false;
    CHECK(plan_add_norm(n).why == NormWhy::kNull);
  }
  in.rows = -1; in.cols = 8; in.x_dtype = 1; in.out_dtype = 1;
  CHECK(plan_add_norm(in).why == NormWhy::kShape);
  in.rows = 0;
  CHECK(plan_add_norm(in).why == NormWhy::kOk && plan_add_norm(in).empty);
  return plans;
}

static NormPoolPlanIn pool_in(int batch, int head, int groups, int mgr, int cols) {
  NormPoolPlanIn in{};
  in.batch = batch; in.head = head; in.groups = groups; in.cols = cols;
  in.group_rows = in.max_group_rows = mgr;
  in.rows = head + groups * mgr;
  in.in_bstride = in.out_bstride = static_cast<long long>(in.rows) * cols;
  in.has_x = in.has_weight = in.has_out = in.has_res = in.has_ws = true;
  in.x_dtype = in.out_dtype = kNormBf16; in.res_dtype = kNormF32;
  in.x_al = in.res_al = in.w_al = in.out_al = true;
  in.workspace_bytes = 4ll * batch * groups * (mgr > 16 ? (mgr + 15) / 16 : 1) * cols;
  return in;
}

static long walk_norm_pool() {
  g_what = "norm_pool batch head*100+groups mgr cols";
  const int Bs[] = {0, 1, 2, 5}, Hs[] = {0, 1, 16, 17, 33}, Gs[] = {1, 2, 3, 8};
  const int Ms[] = {0, 1, 15, 16, 17, 33, 1568};
  const int Cs[] = {4, 192, 256, 260, 576, 1024, 1028, 2048};
  long plans = 0;
  for (int B : Bs) for (int H : Hs) for (int G : Gs) for (int M : Ms) for (int C : Cs)
    for (int dts = 0; dts < 6; ++dts) {
      g_a = B; g_b = H * 100 + G; g_c = M; g_d = C;
      NormPoolPlanIn in = pool_in(B, H, G, M, C);
      // (x, out, res): the fast combination with and without a residual, then four others
      in.x_dtype = dts < 3 || dts == 5; in.out_dtype = dts < 3 || dts == 4;
      in.res_dtype = dts == 2; in.has_res = dts != 1;
      const int slices = M > 16 ? (M + 15) / 16 : 1;
      const NormPoolPlan pl = plan_norm_pool(in);
      ++plans;
      CHECK(pl.why == NormWhy::kOk);
      CHECK(pl.empty == (B == 0 || in.rows == 0));
      CHECK(pl.slices == slices && pl.slices == pool_slices(M) && pl.groups == G);
      CHECK(pl.gx == static_cast<unsigned>(slices > (H + 15) / 16 ? slices : (H + 15) / 16));
      CHECK(pl.gy == static_cast<unsigned>(G) + 1 && pl.gz == static_cast<unsigned>(B));
      CHECK(16ll * pl.gx >= H && 16ll * pl.gx >= M && pl.block == 256);
      CHECK(pl.lds == 16u * static_cast<unsigned>(C));
      const bool fast = dts < 2 && C <= 1024 && (in.rows + 1ll) * C * 4 < (1ll << 31);
      CHECK((pl.family == NormFamily::kFast) == fast);
      CHECK((pl.family == NormFamily::kGeneric) == !fast);
      const int (&set)[4] = fast ? kFastSet : kVecSet;
      CHECK(in_set(pl.cpl, set) && pl.cpl * 256 >= C && pl.cpl == smallest((C + 255) / 256, set));
      // the part regions: back to back from 0, ending exactly at the reported size
      long long next = 0;
      for (int b = 0; b < B; ++b) for (int g = 0; g < G; ++g) for (int s = 0; s < slices; ++s) {
        CHECK(pl.part_offset(b, g, s, C) == next);
        next += C;
      }
      CHECK(next * 4 == pl.workspace_bytes);
      const NormPoolPlan q = plan_norm_pool_shape(B, G, M, C);
      CHECK(q.workspace_bytes == pl.workspace_bytes && q.slices == pl.slices);
      CHECK(pl.workspace_bytes == 4ll * B * G * slices * C);
      // one byte less is refused, no workspace at all is not
      if (pl.workspace_bytes > 0) {
        NormPoolPlanIn less = in;
        less.workspace_bytes = pl.workspace_bytes - 1;
        CHECK(plan_norm_pool(less).why == NormWhy::kWorkspace);
        less.has_ws = false; less.workspace_bytes = 0;
        CHECK(plan_norm_pool(less).why == NormWhy::kOk);
      }
    }
  // the 2^31 switch: (rows + 1) cols 4 < 2^31, at cols 1024 rows 524286 is the last fast one
  g_what = "norm_pool 2^31";
  for (int rows : {524286, 524287}) {
    NormPoolPlanIn in = pool_in(1, 0, 1, rows, 1024);
    g_a = rows;
    CHECK((plan_norm_pool(in).family == NormFamily::kFast) == (rows == 524286));
    CHECK(plan_norm_pool(in).cpl == 4);
  }
  // refusals in order: null, shape / dtype / strides / tiling, alignment, workspace
  g_what = "norm_pool refusals";
  NormPoolPlanIn bad = pool_in(2, 1, 3, 17, 64);
  bad.workspace_bytes -= 1;
  CHECK(plan_norm_pool(bad).why == NormWhy::kWorkspace);
  bad.res_al = false;
  CHECK(plan_norm_pool(bad).why == NormWhy::kAlign);
  NormPoolPlanIn shape = bad;
  shape.cols = 66;
  CHECK(plan_norm_pool(shape).why == NormWhy::kShape);
  shape.has_out = false;
  CHECK(plan_norm_pool(shape).why == NormWhy::kNull);
  int n = 0;
  auto refused = [&](NormPoolPlanIn v) { g_a = n++; CHECK(plan_norm_pool(v).why == NormWhy::kShape); };
  const NormPoolPlanIn ok = pool_in(2, 1, 3, 17, 64);
  CHECK(plan_norm_pool(ok).why == NormWhy::kOk);
  { auto v = ok; v.batch = -1; refused(v); }
  { auto v = ok; v.cols = 0; refused(v); }
  { auto v = ok; v.cols = 2052; v.in_bstride = v.out_bstride = 2052ll * v.rows; refused(v); }
  { auto v = ok; v.head = v.rows + 1; refused(v); }
  { auto v = ok; v.groups = 0; refused(v); }
  { auto v = ok; v.in_bstride -= 4; refused(v); }
  { auto v = ok; v.out_bstride += 2; refused(v); }
  { auto v = ok; v.rev_frame = 5; refused(v); }
  { auto v = ok; v.rev_frame = -1; refused(v); }
  { auto v = ok; v.x_dtype = 2; refused(v); }
  { auto v = ok; v.res_dtype = 2; refused(v); }
  { auto v = ok; v.group_rows = 16; refused(v); }              // groups do not tile the rows
  { auto v = ok; v.max_group_rows = 18; refused(v); }          // implicit groups: mgr == group_rows
  { auto v = ok; v.res_dtype = 2; v.has_res = false; v.res_al = false;
    CHECK(plan_norm_pool(v).why == NormWhy::kOk); }            // an absent residual is not read
  { auto v = ok; v.has_bounds = true; v.group_rows = 0; v.max_group_rows = 40;
    v.workspace_bytes = 4ll * 2 * 3 * 3 * 64;
    CHECK(plan_norm_pool(v).why == NormWhy::kOk && plan_norm_pool(v).slices == 3); }
  { auto v = ok; v.rev_frame = 17; CHECK(plan_norm_pool(v).why == NormWhy::kOk); }
  return plans;
}

static long walk_pool_finish() {
  g_what = "pool_finish mode*10+keep groups mgr cols";
  const int Ms[] = {1, 15, 16, 17, 33, 1568}, Cs[] = {4, 576, 1024, 1028, 2048}, Gs[] = {1, 3, 8};
  long plans = 0;
  for (int mode = 0; mode < 4; ++mode) for (int keep = 0; keep < 2; ++keep)
    for (int G : Gs) for (int M : Ms) for (int C : Cs) for (int B : {0, 1, 3}) {
      g_a = mode * 10 + keep; g_b = G; g_c = M; g_d = C;
      PoolFinishPlanIn in{};
      in.batch = B; in.groups = G; in.max_group_rows = M; in.cols = C; in.mode = mode;
      in.keep_temporal = keep; in.has_ws = in.has_cls = in.has_xpool = true;
      in.cls_dtype = kNormBf16; in.xp_dtype = kNormF32;
      const PoolFinishPlan pl = plan_pool_finish(in);
      ++plans;
      const int navg = keep ? G : 1;
      CHECK(pl.why == NormWhy::kOk && pl.empty == (B == 0));
      CHECK(pl.prow == (mode == kPoolCls ? 1 : mode == kPoolClsCatAvg ? 1 + navg : navg));
      CHECK(pl.gx == static_cast<unsigned>(pl.prow) && pl.gy == static_cast<unsigned>(B));
      CHECK(pl.block == 1024 && pl.slices == (M + 15) / 16);
      CHECK(pl.slices == plan_norm_pool_shape(B, G, M, C).slices);
      // the pointers a mode needs: the workspace unless cls, the CLS rows unless avg
      PoolFinishPlanIn n = in;
      n.has_ws = false;
      CHECK((plan_pool_finish(n).why == NormWhy::kNull) == (mode != kPoolCls));
      n = in; n.has_cls = false;
      CHECK((plan_pool_finish(n).why == NormWhy::kNull) == (mode != kPoolAvg));
      n = in; n.has_xpool = false; n.cols = 6;
      CHECK(plan_pool_finish(n).why == NormWhy::kNull);      // null before shape
      n = in; n.cols = 2052;
      CHECK(plan_pool_finish(n).why == NormWhy::kShape);
      n = in; n.max_group_rows = 0;
      CHECK(plan_pool_finish(n).why == NormWhy::kShape);
      n = in; n.xp_dtype = 2;
      CHECK(plan_pool_finish(n).why == NormWhy::kShape);
      n = in; n.groups = 0;
      CHECK(plan_pool_finish(n).why == NormWhy::kShape);
    }
  PoolFinishPlanIn in{};
  in.batch = 1; in.groups = 1; in.max_group_rows = 1; in.cols = 4; in.has_ws = in.has_xpool = true;
  for (int mode : {-1, 4}) {
    in.mode = mode;
    g_a = mode;
    CHECK(plan_pool_finish(in).why == NormWhy::kShape);
  }
  return plans;
}

int main() {
  static_assert(pool_slices(0) == 1 && pool_slices(1) == 1 && pool_slices(16) == 1 &&
                pool_slices(17) == 2 && pool_slices(1568) == 98, "pool_slices");
  static_assert(kPoolRB == 16 && kSmallStoreRows == 32768 && kNormMaxCols == 2048 &&
                kNormFastMaxCols == 1024 && kNorm2G == 2147483648ll, "limits");
  const long a = walk_add_norm(), b = walk_norm_pool(), c = walk_pool_finish();
  std::printf("%ld + %ld + %ld plans, %ld failures\n", a, b, c, g_fail);
  return g_fail ? 1 : 0;
}

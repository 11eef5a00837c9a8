// Stand-alone check of the selective scan's host plan (videomamba_amd/csrc/vm_scan_plan.h):
// walks plan_scan() over a grid of shapes, CU counts, operand facts and buffer offers and
// exits non-zero unless every plan is self-consistent and vm_selective_scan_dtproj_fits'
// answer (scan_dtproj_route and the two geometry rules) is the one the rules written out give.  Built and run by
// tests/test_api_cpu.py with -fsanitize=address,undefined; needs no GPU and no HIP.
#include <cstdio>

#include "vm_scan_plan.h"

using namespace vm;

static long g_fail = 0;
static const ScanPlanIn* g_in = nullptr;
#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      if (g_fail++ < 20)                                                                     \
        std::fprintf(stderr,                                                                 \
                     "line %d: %s  [B=%d D=%d L=%d seg=%d es=%d sgpr=%d bc1=%d pair=%d "     \
                     "dtp=%d cus=%d dev=%d ws=%zu sync=%zu]\n",                              \
                     __LINE__, #cond, g_in->batch, g_in->dim, g_in->seqlen, g_in->segments,  \
                     g_in->es, g_in->sgpr_bc, g_in->bc1, g_in->pair, g_in->dtp, g_in->cus,   \
                     g_in->dev_cus, g_in->ws_offer, g_in->sync_offer);                       \
    }                                                                                        \
  } while (0)

int main() {
  const int Bs[] = {1, 2, 4, 8, 71, 72};
  const int Ds[] = {64, 100, 1152, 1536};
  const int Ls[] = {0, 1, 8, 63, 64, 65, 197, 1569, 3137, 12545};
  const int Ss[] = {0, 1, 4, 7, 20, 24, 300, 5000};
  const int Cus[] = {64, 256, 304};
  const int Dev[] = {0, 64, 256};
  const int Es[] = {2, 4};
  long plans = 0, seen[4] = {0, 0, 0, 0}, seen_lbc = 0, fits[4] = {0, 0, 0, 0};
  for (int B : Bs) for (int D : Ds) for (int L : Ls) for (int seg : Ss) for (int cus : Cus) {
    // what the ABI size queries report: no operands, everything on offer
    ScanPlanIn qi{};
    qi.batch = B; qi.dim = D; qi.seqlen = L; qi.segments = seg; qi.es = 2;
    qi.sgpr_bc = qi.bc1 = true; qi.cus = cus;
    qi.ws_offer = qi.sync_offer = ~static_cast<size_t>(0);
    g_in = &qi;
    const ScanPlan q = plan_scan(qi);
    CHECK((q.ws_query == 0) == (q.chosen <= 1) && (q.sync_query == 0) == (q.chosen <= 1));
    const size_t ws_offers[] = {0, q.ws_query ? q.ws_query - 1 : 0, q.ws_query};
    const size_t sync_offers[] = {0, q.sync_query ? q.sync_query - 1 : 0, q.sync_query};
    for (int dev : Dev) for (int es : Es) for (int flags = 0; flags < 16; ++flags)
    for (size_t ws : ws_offers) for (size_t sy : sync_offers) {
      ScanPlanIn in = qi;
      in.es = es; in.dev_cus = dev; in.ws_offer = ws; in.sync_offer = sy;
      in.sgpr_bc = flags & 1; in.bc1 = flags & 2; in.pair = flags & 4; in.dtp = flags & 8;
      g_in = &in;
      const ScanPlan pl = plan_scan(in);
      ++plans;
      ++seen[static_cast<int>(pl.form)];
      seen_lbc += pl.lbc;
      const size_t b = B, d = D, groups = (D + 63) / 64;
      // the size queries do not depend on the operands or the offers
      CHECK(pl.ws_query == q.ws_query && pl.sync_query == q.sync_query && pl.chosen == q.chosen);
      // (a) workspace regions in order, disjoint, inside the plan's bytes <= the query's
      CHECK(pl.ws_bytes <= q.ws_query && pl.ws_bytes <= in.ws_offer);
      CHECK(pl.sync_bytes <= q.sync_query && pl.sync_bytes <= in.sync_offer);
      if (pl.chunked()) {
        const size_t nb = b * pl.nblk;
        CHECK(pl.segE == 0 && pl.segE + nb * kChW * d * kMaxN <= pl.segP);
        CHECK(pl.segP + nb * kChW * d <= pl.aggH);
        CHECK(pl.aggH + nb * d * kMaxN <= pl.aggS);
        CHECK((pl.aggS + nb * d) * sizeof(float) <= pl.ws_bytes);
      } else if (pl.form == ScanForm::kLegacy) {
        const size_t rows = b * pl.S * d;
        CHECK(pl.hend == 0 && pl.hend + rows * kMaxN <= pl.hin);
        CHECK(pl.hin + rows * kMaxN <= pl.sdel);
        CHECK((pl.sdel + rows) * sizeof(float) <= pl.ws_bytes);
      } else {
        CHECK(pl.ws_bytes == 0 && pl.sync_bytes == 0);
      }
      // (b) the segments cover the sequence, none is empty
      const int Lmin1 = L > 1 ? L : 1;
      CHECK(pl.S >= 1 && pl.S <= Lmin1);
      CHECK(pl.T == pl.seg_len && static_cast<long long>(pl.S) * pl.T >= L);
      CHECK(static_cast<long long>(pl.S - 1) * pl.T < Lmin1);
      CHECK(static_cast<long long>(pl.nblk) * kChW * pl.T >= L);
      CHECK(static_cast<long long>(pl.nblk) * kChW >= pl.S);
      // (c) one launch: the whole grid resident, and the sync buffer
      if (pl.form == ScanForm::kChunk1) {
        const size_t need = kSyncHeaderWords * sizeof(unsigned) +
                            b * groups * pl.nblk * (kMaxN + 1) * 64 * sizeof(unsigned long long);
        CHECK(static_cast<long long>(groups) * pl.nblk * B <= dev);
        CHECK(pl.sync_bytes >= need && in.sync_offer >= need);
      } else {
        CHECK(pl.sync_bytes == 0);
      }
      // (d) LBC and DTP limits
      if (pl.lbc)
        CHECK(pl.form == ScanForm::kChunk1 && in.dtp && in.bc1 && kChW * pl.T <= kChLbcRows);
      if (in.dtp && pl.chunked()) CHECK(pl.T <= kChDtpT && in.bc1);
      if (in.dtp) CHECK(pl.form != ScanForm::kLegacy);
      // (e) legacy: LDS-staged B / C only, bounded segment count, never a pair
      if (pl.form == ScanForm::kLegacy) CHECK(!in.sgpr_bc && pl.S <= kMaxSeg && !in.pair);
      if (pl.chunked()) CHECK(in.sgpr_bc);
      // (f) too little workspace: the single pass
      if (in.ws_offer < q.ws_query) CHECK(pl.form == ScanForm::kSingle);
      if (pl.form == ScanForm::kSingle) CHECK(pl.S == 1 && pl.T == L);
      // (g) vm_selective_scan_dtproj_fits: the four-way answer against the rules of
      // seq_dtp_supported / seq_dtp_chunk_supported written out (literal numbers), for every
      // dt_rank, state count, padded W_dt width and verdict of the operand checks
      if (!in.dtp) continue;
      const int Rs[] = {0, 4, 6, 12, 32, 36, 64, 68};
      const int Ns[] = {8, 16};
      const int Wds[] = {16, 32, 48, 64};
      for (int R : Rs) for (int N : Ns) for (int wd : Wds) for (int ops = 0; ops < 2; ++ops) {
        const bool rank_ok = R >= 1 && R % 4 == 0;
        const bool single = N == 16 && D % 128 == 0 && rank_ok && R <= 64 &&
                            wd >= 16 * ((R + 15) / 16) && wd % 4 == 0;
        const bool chunk = pl.chunked() && N == 16 && (wd == 32 || wd == 64) && rank_ok && R <= wd;
        CHECK(scan_dtp_single_geom(D, N, R, wd) == single);
        CHECK(scan_dtp_chunk_geom(pl, N, R, wd) == chunk);
        int want;
        if (pl.chosen <= 1) {
          want = single && ops ? 1 : 0;
        } else if (!(chunk && ops)) {
          want = 0;  // a segmented request never falls back to the single pass
        } else {
          const long long wgs = static_cast<long long>((D + 63) / 64) * pl.nblk * B;
          want = wgs <= dev ? 3 : 2;
          CHECK(pl.T <= 64);
          // the one-launch form runs exactly where the answer is 3 and the sync buffer is there
          CHECK((pl.form == ScanForm::kChunk1) == (want == 3 && in.sync_offer >= q.sync_query));
        }
        const int got = scan_dtproj_route(pl, single && ops, chunk && ops, B, D, dev);
        CHECK(got == want);
        ++fits[got];
      }
    }
  }
  // the walk reached every form
  for (int f = 0; f < 4; ++f) {
    if (!seen[f]) {
      std::fprintf(stderr, "form %d never planned\n", f);
      ++g_fail;
    }
  }
  for (int a = 0; a < 4; ++a) {
    if (!fits[a]) {
      std::fprintf(stderr, "dtproj fits answer %d never given\n", a);
      ++g_fail;
    }
  }
  if (!seen_lbc) {
    std::fprintf(stderr, "LBC never planned\n");
    ++g_fail;
  }
  std::printf("dtproj fits: %ld refused, %ld single, %ld segmented, %ld segmented resident\n",
              fits[0], fits[1], fits[2], fits[3]);
  std::printf("%ld plans: single %ld legacy %ld chunk2 %ld chunk1 %ld lbc %ld, %ld failures\n",
              plans, seen[0], seen[1], seen[2], seen[3], seen_lbc, g_fail);
  return g_fail ? 1 : 0;
}

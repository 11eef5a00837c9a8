// Host-side plan of a token-major selective scan (vm_scan_seq.hip): which form runs, its
// geometry, and where every region of the caller's workspace lies.  Plain C++17, no HIP
// header: the size queries, the support checks and the launches of vm_scan_seq.hip all read
// one ScanPlan, and tests/host/scan_plan_check.cpp walks plan_scan() over a grid of shapes
// on the host.
//
// CU counts: the ABI size queries plan for the current device (kCalibCUs without one).  A
// launch entry plans once, for its stream's device, and uses that plan for its checks and
// its launch alike.  Where every device of a machine has the same CU count the two agree.
#pragma once

#include <cstddef>

namespace vm {

constexpr int kMaxN = 16;     // states per channel
constexpr int kSeqNW = 2;     // single pass: waves (channel groups of 64) per workgroup
constexpr int kChW = 8;  // segments (waves) per workgroup
constexpr int kMaxSeg = 256;  // segments per sequence (legacy form)
constexpr int kChLbcRows = 256;  // steps per block the LDS B|C staging (LBC) holds
constexpr int kChDtpT = 64;      // max segment length with dt_proj inside
constexpr int kSyncHeaderWords = 4;  // error word, epoch, start count, pad
constexpr int kCalibCUs = 256;  // the part the cost model below was swept on

// Segment count.  A chip-filling batch (>= 1,280 waves of 64-channel groups) runs
// single-pass.  Below that the chunked form's time is modelled from a sweep of forced
// segment counts at M-16f geometry (scripts/diag/scan_segments_sweep.py, B = 1 .. 64,
// L = 3,137 and 12,545; profiles/r02_scan_segments_sweep.jsonl):
//   time ~ 16.6 us + 0.69 us x k x T + 0.43 us x nblk
// with T steps per segment, nblk = blocks of kChW segments per sequence and
// k = ceil(workgroups / 256): a CU holding k of the 512-thread workgroups runs their waves'
// steps k-fold interleaved (the passes are issue-bound), and every block adds one aggregate
// to the entry walk.  The model is within ~6 % of the sweep; the round-1 rule (a fixed
// ~1,792-wave target) picked 2-3x slower counts at B >= 4 (T = 126 .. 1,569 steps).
// Depends on (batch, dim, seqlen) and the device's CU count only (the sweep ran on a
// 256-CU MI355X; `cus` rescales k and the chip-filling threshold for other parts).
inline int choose_segments(int batch, int dim, int seqlen, int cus) {
  if (seqlen < 64) return 1;
  const long long groups = (dim + 63) / 64;
  if (batch * groups >= 5 * cus) return 1;
  const int max_s = (seqlen + 7) / 8;  // segments of at least 8 steps
  int best = 1;
  double best_cost = 1e30;
  for (int S = 2; S <= max_s && S <= 2048; S += (S < 64 ? 1 : 8)) {
    const int T = (seqlen + S - 1) / S;
    const int segs = (seqlen + T - 1) / T;
    const long long nblk = (segs + kChW - 1) / kChW;
    const long long k = (batch * groups * nblk + cus - 1) / cus;
    const double cost = 0.69 * static_cast<double>(k * T) + 0.43 * static_cast<double>(nblk);
    if (cost < best_cost) {
      best_cost = cost;
      best = S;
    }
  }
  return best;
}

// Workgroups of the chunked form: one per (64-channel group, block of kChW segments, batch
// row).  The one-launch form needs them all resident at one workgroup per CU; the mixer folds
// dt_proj into a segmented scan only where they are (vm_selective_scan_dtproj_fits).
constexpr long long scan_chunk_grid(int batch, int dim, int nblk) {
  return static_cast<long long>((dim + 63) / 64) * nblk * batch;
}

enum class ScanForm {
  kSingle,  // one pass per (batch row, 128 channels)
  kLegacy,  // summary / carry / final (LDS-staged B / C)
  kChunk2,  // chunked, PASS 1 and PASS 2 as two launches
  kChunk1,  // chunked, one launch handing block aggregates on through the sync buffer
};

struct ScanPlanIn {
  int batch, dim, seqlen;
  int segments;  // > 0 forces the segment count (tests and sweeps), 0 = the cost model
  int es;        // element size in bytes
  bool sgpr_bc;  // B / C rows can come in as scalar loads
  bool bc1;      // C directly follows B in the row
  bool pair;     // paired (bidirectional) scan
  bool dtp;      // dt_proj inside the scan
  int cus;       // CU count the cost model sizes for
  int dev_cus;   // CU count of the launch device, 0 if unknown (no one-launch form then)
  size_t ws_offer, sync_offer;  // bytes of workspace / zeroed sync buffer on offer
};

struct ScanPlan {
  ScanForm form;
  int chosen;   // segment count asked for (> 1: a segmented form, given the workspace)
  int S;        // segments that run, every one non-empty
  int T;        // steps per segment (== seg_len)
  int nblk;     // blocks of kChW segments per sequence
  int seg_len;
  bool lbc;     // the block's B|C rows staged in LDS (one-launch DTP)
  // what the ABI size queries report: they do not see the operands, so the larger of the
  // chunked and the legacy need
  size_t ws_query, sync_query;
  size_t ws_bytes, sync_bytes;  // what `form` uses of the buffers on offer
  // workspace regions, in floats from the workspace base
  size_t segE, segP, aggH, aggS;  // chunked (ChunkWork)
  size_t hend, hin, sdel;         // legacy (SeqWork)
  bool chunked() const { return form == ScanForm::kChunk2 || form == ScanForm::kChunk1; }
};

inline ScanPlan plan_scan(const ScanPlanIn& in) {
  ScanPlan pl{};
  const int L = in.seqlen;
  // the requested count, at most one segment per step
  int S = in.segments > 0 ? in.segments : choose_segments(in.batch, in.dim, L, in.cus);
  if (S > L) S = L > 0 ? L : 1;
  if (S < 1) S = 1;
  pl.chosen = S;
  pl.form = ScanForm::kSingle;
  pl.S = 1;
  pl.T = pl.seg_len = L;
  pl.nblk = 1;
  if (S <= 1) return pl;

  // chunked geometry and layout for the requested count
  const size_t groups = static_cast<size_t>((in.dim + 63) / 64);
  const size_t dim = static_cast<size_t>(in.dim);
  const int cT = (L + S - 1) / S;
  const int cS = (L + cT - 1) / cT;
  const int cblk = (cS + kChW - 1) / kChW;
  const size_t nb = static_cast<size_t>(in.batch) * cblk;
  const size_t c_segP = nb * kChW * dim * kMaxN;
  const size_t c_aggH = c_segP + nb * kChW * dim;
  const size_t c_aggS = c_aggH + nb * dim * kMaxN;
  const size_t c_bytes = (c_aggS + nb * dim) * sizeof(float);
  // legacy geometry and layout (regions sized for the clamped requested count)
  const int lS = S > kMaxSeg ? kMaxSeg : S;
  const int lT = (L + lS - 1) / lS;
  const size_t states = static_cast<size_t>(in.batch) * lS * dim * kMaxN;
  const size_t l_bytes = (2 * states + static_cast<size_t>(in.batch) * lS * dim) * sizeof(float);

  pl.ws_query = c_bytes > l_bytes ? c_bytes : l_bytes;
  pl.sync_query = kSyncHeaderWords * sizeof(unsigned) +
                  static_cast<size_t>(in.batch) * groups * cblk * (kMaxN + 1) * 64 *
                      sizeof(unsigned long long);
  if (in.ws_offer < pl.ws_query) return pl;  // too little workspace: the single pass

  if (in.sgpr_bc) {
    // dt_proj inside the chunked scan: bc1 rows and a segment that fits the LDS dt block
    if (in.dtp && !(in.bc1 && cT <= kChDtpT)) return pl;
    // one launch needs the zeroed sync buffer and every block it waits on resident: the
    // whole grid at one workgroup per CU
    const bool one = in.sync_offer >= pl.sync_query &&
                     scan_chunk_grid(in.batch, in.dim, cblk) <= in.dev_cus;
    pl.form = one ? ScanForm::kChunk1 : ScanForm::kChunk2;
    pl.S = cS;
    pl.T = pl.seg_len = cT;
    pl.nblk = cblk;
    pl.lbc = one && in.dtp && in.bc1 && in.es == 2 && kChW * cT <= kChLbcRows;
    pl.ws_bytes = c_bytes;
    pl.sync_bytes = one ? pl.sync_query : 0;
    pl.segP = c_segP;
    pl.aggH = c_aggH;
    pl.aggS = c_aggS;
    return pl;
  }
  // LDS-staged B / C: a paired or DTP scan is never legacy (their entries reject it)
  if (in.pair || in.dtp) return pl;
  pl.form = ScanForm::kLegacy;
  pl.T = pl.seg_len = lT;
  pl.S = (L + lT - 1) / lT;
  pl.nblk = (pl.S + kChW - 1) / kChW;
  pl.ws_bytes = l_bytes;
  pl.hin = states;
  pl.sdel = 2 * states;
  return pl;
}

// dt_proj inside the scan (vm_selective_scan_dtproj_fwd): the limits of its two forms that
// the geometry alone decides.  What depends on the operands (strides, alignment, 31-bit
// extents) is seq_dtp_supported's and seq_dtp_chunk_supported's, which call these.
// `wdt_ld`: columns of the zero-padded W_dt.
constexpr bool scan_dtp_single_geom(int dim, int dstate, int dt_rank, int wdt_ld) {
  return dstate == kMaxN && dim % (64 * kSeqNW) == 0 && dt_rank >= 1 && dt_rank <= 64 &&
         dt_rank % 4 == 0 && wdt_ld >= 16 * ((dt_rank + 15) / 16) && wdt_ld % 4 == 0;
}
// `pl` planned with dtp: chunked only for scalar-load B|C rows with C directly after B,
// segments of at most kChDtpT steps and enough workspace.
inline bool scan_dtp_chunk_geom(const ScanPlan& pl, int dstate, int dt_rank, int wdt_ld) {
  return pl.chunked() && dstate == kMaxN && (wdt_ld == 32 || wdt_ld == 64) && dt_rank >= 1 &&
         dt_rank <= wdt_ld && dt_rank % 4 == 0;
}
// What vm_selective_scan_dtproj_fwd does with a call, and vm_selective_scan_dtproj_fits
// answers: 0 refused, 1 the single pass, 2 the segmented form on a grid past `dev_cus`, 3 the
// segmented form with the whole grid resident at one workgroup per CU.  `single_ok` /
// `chunk_ok`: what the two support checks said of the operands.
inline int scan_dtproj_route(const ScanPlan& pl, bool single_ok, bool chunk_ok, int batch,
                             int dim, int dev_cus) {
  if (pl.chosen <= 1) return single_ok ? 1 : 0;
  if (!chunk_ok) return 0;
  return scan_chunk_grid(batch, dim, pl.nblk) <= dev_cus ? 3 : 2;
}

}  // namespace vm

// Host-side plan of the selective scan's backward (vm_scan_bwd.hip): the chunk length of
// its recompute sweeps and where every region of the caller's workspace lies.  Plain C++17,
// no HIP header: the size query, the entry's workspace check and the launch all read one
// ScanBwdPlan, and tests/host/scan_bwd_plan_check.cpp walks plan_scan_bwd() over a grid of
// shapes on the host.
//
// One workgroup of kBwdWaves waves owns (batch row, 64 channels): a lane per channel, each
// wave kBwdNS of the 16 states, walking the sequence in chunks of kBwdT steps.
// Workspace regions, in floats from the workspace base (dpad = 64 * groups):
//   ckpt  [batch][nchunks - 1][groups][16][64]  the state entering chunks 1 .. nchunks - 1
//                                               (chunk 0 enters with h0, an input)
//   bc    [batch][groups][seqlen][32]           per-group partial sums of dB (0..15) | dC
//   pa    [batch][dpad][16]                     per-batch-row partial sums of dA
//   pd    [batch][dpad]                         ... of dD
//   pb    [batch][dpad]                         ... of ddelta_bias
// In bytes: 64 (nchunks - 1) + 2 seqlen + 72 per (batch row, padded channel), with
// nchunks - 1 < seqlen / kBwdT: under 10 batch seqlen dpad + 72 batch dpad.
#pragma once

#include <cstddef>

namespace vm {

constexpr int kBwdN = 16;     // states per channel
constexpr int kBwdT = 8;      // steps per chunk: 8 x 16 states x 64 lanes x 4 B = 32 KiB of LDS
constexpr int kBwdLanes = 64;  // channels per workgroup, one per lane of each wave
constexpr int kBwdWaves = 4;   // waves per workgroup
constexpr int kBwdNS = kBwdN / kBwdWaves;  // states per wave

struct ScanBwdPlan {
  int T;        // steps per chunk
  int nchunks;  // chunks per sequence, every one non-empty (0 for an empty sequence)
  int groups;   // 64-channel groups
  int dpad;     // channels rounded up to whole groups
  size_t ckpt, bc, pa, pd, pb;  // region offsets in floats
  size_t ws_bytes;
  // steps [begin, end) of chunk c
  int chunk_begin(int c) const { return c * T; }
  int chunk_end(int c, int seqlen) const { return (c + 1) * T < seqlen ? (c + 1) * T : seqlen; }
  // floats per region
  size_t ckpt_floats(int batch) const {
    return static_cast<size_t>(batch) * (nchunks > 1 ? nchunks - 1 : 0) * groups * kBwdN * kBwdLanes;
  }
  size_t bc_floats(int batch, int seqlen) const {
    return static_cast<size_t>(batch) * groups * seqlen * 2 * kBwdN;
  }
};

inline ScanBwdPlan plan_scan_bwd(int batch, int dim, int seqlen) {
  ScanBwdPlan pl{};
  if (batch < 0) batch = 0;
  if (dim < 0) dim = 0;
  if (seqlen < 0) seqlen = 0;
  pl.T = kBwdT;
  pl.nchunks = (seqlen + kBwdT - 1) / kBwdT;
  pl.groups = (dim + kBwdLanes - 1) / kBwdLanes;
  pl.dpad = pl.groups * kBwdLanes;
  const size_t rows = static_cast<size_t>(batch) * pl.dpad;
  pl.ckpt = 0;
  pl.bc = pl.ckpt + pl.ckpt_floats(batch);
  pl.pa = pl.bc + pl.bc_floats(batch, seqlen);
  pl.pd = pl.pa + rows * kBwdN;
  pl.pb = pl.pd + rows;
  pl.ws_bytes = (pl.pb + rows) * sizeof(float);
  return pl;
}

}  // namespace vm

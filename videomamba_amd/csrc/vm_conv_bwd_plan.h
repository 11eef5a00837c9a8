// Host-side plan of the causal conv1d backward (vm_conv_bwd.hip): the time tiles, the layout
// of the dweight / dbias partials in the caller's workspace and the ranges the second kernel
// adds them in.  Plain C++17, no HIP header: the size query, the entry's workspace check and
// both launches read one ConvBwdPlan, and tests/host/conv_bwd_plan_check.cpp walks
// plan_conv_bwd() over a grid of shapes on the host.  It takes (batch, dim, seqlen, width)
// only, so the order of every sum is the same on every device.
//
// One 64-thread workgroup owns (batch row, time tile, 64 channel runs).  A tile is kCbTT
// steps of dx; the walk over it covers kCbTT + kCbWM - 1 = 64 steps (eight 8-row loads),
// because dx[j] needs dpre at up to kCbWM - 1 steps ahead of j.
// Workspace, in floats from the workspace base (dpad = round_up(dim, 64)):
//   part [batch * tiles][width + 1][dpad]   slot i < width: the tile's sum of
//                                           dpre[t] * e[t - width + 1 + i]; slot width: of dpre[t]
// In bytes 4 batch tiles (width + 1) dpad with tiles = ceil(seqlen / 61): at most
// 20 batch dpad (seqlen / 61 + 1).
// The reduce kernel gives one thread (channel, slot, range r): it adds parts
// [r per_range, (r + 1) per_range) in index order, then the kCbRanges range sums are added in
// range order.
#pragma once

#include <cstddef>

namespace vm {

constexpr int kCbWM = 4;       // taps the kernel is unrolled for (width <= kCbWM, right-aligned)
constexpr int kCbTT = 61;      // dx steps per time tile
constexpr int kCbWalk = kCbTT + kCbWM - 1;  // steps a tile walks: 64
constexpr int kCbLanes = 64;   // threads per workgroup, one channel run each
constexpr int kCbRanges = 16;  // contiguous part ranges of the reduce kernel

struct ConvBwdPlan {
  int tiles;      // time tiles per batch row (0 for an empty sequence)
  int slots;      // width + 1
  int dpad;       // channels rounded up to 64
  long long parts;      // batch * tiles
  long long per_range;  // parts per reduce range (the last ranges may be short or empty)
  size_t ws_bytes;
  constexpr int tile_begin(int i) const { return i * kCbTT; }
  constexpr int tile_end(int i, int seqlen) const {
    return (i + 1) * kCbTT < seqlen ? (i + 1) * kCbTT : seqlen;
  }
  // float offset of channel 0 of (part, slot)
  constexpr size_t part_offset(long long part, int slot) const {
    return (static_cast<size_t>(part) * slots + slot) * dpad;
  }
  constexpr long long range_begin(int r) const {
    const long long v = r * per_range;
    return v < parts ? v : parts;
  }
  constexpr long long range_end(int r) const { return range_begin(r + 1); }
};

inline ConvBwdPlan plan_conv_bwd(int batch, int dim, int seqlen, int width) {
  ConvBwdPlan pl{};
  if (batch < 0) batch = 0;
  if (dim < 0) dim = 0;
  if (seqlen < 0) seqlen = 0;
  if (width < 1) width = 1;
  if (width > kCbWM) width = kCbWM;
  pl.tiles = (seqlen + kCbTT - 1) / kCbTT;
  pl.slots = width + 1;
  pl.dpad = (dim + kCbLanes - 1) / kCbLanes * kCbLanes;
  pl.parts = dim > 0 ? static_cast<long long>(batch) * pl.tiles : 0;
  pl.per_range = (pl.parts + kCbRanges - 1) / kCbRanges;
  pl.ws_bytes = static_cast<size_t>(pl.parts) * pl.slots * pl.dpad * sizeof(float);
  return pl;
}

}  // namespace vm

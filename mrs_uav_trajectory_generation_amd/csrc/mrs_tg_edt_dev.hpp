// mrs_tg_edt_dev.hpp -- what the y and z passes of the full distance transform (mrs_tg_edt.hip) and of the update of a changed box
// (mrs_tg_edt_region.hip) share on the device: the staged tile of a workgroup, its scan, and the value a pass leaves at a node.
// The passes differ in where a tile comes from and where a node goes, which stays with each of them.
#pragma once
#include <hip/hip_runtime.h>

#include "mrs_tg_edt.hpp"

#ifndef MRS_TG_EDT_THREADS
#define MRS_TG_EDT_THREADS 512  // of a workgroup of the y and z passes (an experiment build may say 256 or 1024)
#endif

namespace mrs_tg {

constexpr int kEdtThreads = MRS_TG_EDT_THREADS;
constexpr long long kEdtBlocks = 1 << 20;      // workgroups of a launch at the most

// the staged tile of one workgroup: n rows of tx columns at base + l stride + c, c < width
struct Tile {
  size_t base, stride;
  int n, tx_log2, width;
};

__device__ inline void stage_tile(const double* D, const Tile& T, double* __restrict__ s_tile) {
  const int total = T.n << T.tx_log2, mask = (1 << T.tx_log2) - 1;
  for (int e = threadIdx.x; e < total; e += kEdtThreads) {
    const int l = e >> T.tx_log2, c = e & mask;
    if (c < T.width) s_tile[e] = D[T.base + (size_t)l * T.stride + (size_t)c];
  }
}

// the scan of node (l, c) of the staged tile as a node of the class `occupied`: a node of its own class shows its partial
// distance, a node of the other class is a source at 0 (edtq::seen_by)
__device__ inline double scan_tile(const double* __restrict__ s_tile, const Tile& T, int l, int c, bool occupied, double w,
                                   double limit) {
  const int shift = T.tx_log2;
  return edtq::scan_line([&](int p) { return edtq::seen_by(s_tile[(p << shift) + c], occupied); }, T.n, l, w, limit);
}

// What a pass along y (Last = false) or z (Last = true) leaves at `out` for node (l, c) of the staged tile, element e = (l <<
// tx_log2) + c.  An occupied node of an unsigned field keeps what it holds through the y pass (its -0.0) and becomes 0.0 in the
// last.
template <bool Last>
__device__ inline void tile_node(double* out, const double* __restrict__ s_tile, const Tile& T, int l, int c, int e, double w,
                                 double limit, double max_distance, bool is_signed) {
  const bool occupied = edtq::packed_occupied(s_tile[e]);
  if (occupied && !is_signed) {
    if (Last) *out = 0.0;
  } else {
    const double d = scan_tile(s_tile, T, l, c, occupied, w, limit);
    *out = !Last ? edtq::packed(d, occupied) : (occupied ? edtq::occupied_value(d, max_distance) : edtq::free_value(d, max_distance));
  }
}

inline int edt_log2_of(int power_of_two) {
  int s = 0;
  while ((1 << s) < power_of_two) ++s;
  return s;
}

inline unsigned edt_blocks_for(long long items) { return (unsigned)(items < kEdtBlocks ? items : kEdtBlocks); }

}  // namespace mrs_tg

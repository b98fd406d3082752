// mrs_tg_batch.hpp -- the structure of a batch and its addressing: which path a segment, a vertex or a position of the launch
// belongs to, and where a path starts.  One copy for every kernel and launcher, host-checkable (plain
// C++17 without a HIP include; tests/host/batch_harness.cpp runs it on the CPU against a linear scan of seg_offsets).
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {

// Device-resident structure of a batch (built once per plan).
struct BatchView {
  int n_paths;
  int n_segments;            // sum of S over the batch
  int max_segments;          // largest S
  int uniform_S;             // S if every path has the same segment count, else 0
  const int32_t* seg_offsets;  // [n_paths + 1] CSR over segments (caller's path order)
  const int32_t* order;        // [n_paths] position q -> path index, sorted by S descending (stable)
  const int32_t* slot_start;   // [max_segments + 1] slot_start[j] = number of (q, j') pairs with j' < j
};

// the largest p with first[p] <= x, first[p] = seg_offsets[p] + extra * p (extra 1: a path's first vertex; 0: its first
// segment): a division for uniform batches (instead of log2(P) dependent loads), a binary search over seg_offsets otherwise
MRS_TG_HD inline int path_of(const BatchView& b, int x, int extra) {
  if (b.uniform_S > 0) return x / (b.uniform_S + extra);
  int lo = 0, hi = b.n_paths;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (b.seg_offsets[mid] + extra * mid <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}
// the path of CSR segment s / of vertex v (a path of S segments has S + 1 vertices, the batch sum S + n_paths)
MRS_TG_HD inline int path_of_segment(const BatchView& b, int s) { return path_of(b, s, 0); }
MRS_TG_HD inline int path_of_vertex(const BatchView& b, int v) { return path_of(b, v, 1); }

// a path's first segment, its number of segments (seg0 = first_segment(b, p)) and its first vertex
MRS_TG_HD inline int first_segment(const BatchView& b, int p) { return b.uniform_S > 0 ? p * b.uniform_S : b.seg_offsets[p]; }
MRS_TG_HD inline int segments_of(const BatchView& b, int p, int seg0) {
  return b.uniform_S > 0 ? b.uniform_S : b.seg_offsets[p + 1] - seg0;
}
MRS_TG_HD inline int first_vertex(const BatchView& b, int p) { return first_segment(b, p) + p; }

// the path at position q of a launch (the longest-first order)
struct PathRef {
  int p;   // path index in the caller's order
  int s0;  // first segment (CSR)
  int S;   // number of segments
  int v0;  // first vertex
};

MRS_TG_HD inline PathRef path_at(const BatchView& b, int q) {
  PathRef r;
  if (b.uniform_S > 0) {  // every path has the same segment count: the stable sort left the order alone, offsets are arithmetic
    r.p = q;              // (no dependent loads before a kernel can touch its inputs)
    r.S = b.uniform_S;
    r.s0 = q * b.uniform_S;
    r.v0 = r.s0 + q;
    return r;
  }
  r.p = b.order[q];
  r.s0 = b.seg_offsets[r.p];
  r.S = b.seg_offsets[r.p + 1] - r.s0;
  r.v0 = r.s0 + r.p;
  return r;
}

}  // namespace mrs_tg

// mrs_tg_clearance.hpp -- the mutual clearance within groups of paths (mrs_tg_plan_mutual_clearance, mutual_clearance_kernel) and
// its backward pass (mrs_tg_plan_mutual_clearance_vjp, mutual_clearance_vjp_kernel); DESIGN.md section 11i.  The paths of a plan
// are partitioned into GROUPS (swarms), contiguous runs of paths in the caller's order given by group_offsets [n_groups + 1].
// All paths share the sampling dt; row r of path p sits at the common step first_step[p] + r.  For a live row (p, r) at step s
//   clearance = min over the other paths j of p's group with a live row at step s of
//               c = sqrt((dx dx + dy dy) + (kappa dz)(kappa dz)),   d = row_p - row_j,   kappa = z_scale
// taken with a strict < from +inf in increasing j (a tie goes to the lowest path index, a distance that is not a number never
// becomes a minimum), and partner = the j that gave it, -1 where the clearance is +inf.  No product is contracted into a fused
// multiply-add, so the CPU and the GPU produce the same bits.  Plain double, __host__ __device__, on mrs_tg_hd.hpp alone:
// tests/host/clearance_harness.cpp runs this file under g++.
//
// Backward, the partners held fixed.  With g = dL/dclearance of row (i, .) at step s, j its partner and d = row_i - row_j:
//   g dc/drow_i = (g (dx / c), g (dy / c), g ((kappa (kappa dz)) / c))        row_vjp: each quotient rounded, then the product
//   g dc/drow_j = 0.0 - that, entry by entry                                    partner_row
// g == 0 and c == 0 contribute exactly 0.  THE ORDER OF THE SUMS: row (j, r) at step s has one accumulator per coordinate; it
// starts at 0.0 and takes first the row's own term against its own partner, then, in increasing path index i over the group
// with i != j, the partner_row of every i whose row at step s names j as its partner.  Every addition is accumulate.  A partner
// entry that is -1, lies outside the row's own group, is the row's own path or names a path without a live row at step s
// (partner_in_group, row_at_step) contributes exactly 0 and is never dereferenced.
//
// Out of scope.  A path counts only on the steps where it has rows: "the UAV hovers at its last row" is the caller's padding
// (repeat the last row up to the horizon and raise n_samples).  No gradient flows through the choice of the partner.  Groups
// that are not contiguous runs of paths are not expressible.
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace clrq {

using mrs_tg::accumulate;

// +inf, the clearance of a row without a neighbour: the neutral value of relu(R - c)
MRS_TG_HD inline double no_clearance() {
  MRS_TG_NO_CONTRACT
  return HUGE_VAL;
}

// the live rows of a path: min(n_samples, capacity), none for a dead path
MRS_TG_HD inline int live_rows(bool live, int n_samples, int capacity) {
  MRS_TG_NO_CONTRACT
  const int n = live ? (n_samples < capacity ? n_samples : capacity) : 0;
  return n < 0 ? 0 : n;
}

// the common step of row r of a path whose row 0 sits at step `first` (64-bit: first in [-2^30, 2^30], r below 2^31)
MRS_TG_HD inline long long step_of(int first, int r) {
  MRS_TG_NO_CONTRACT
  return (long long)first + (long long)r;
}

// the live-row-at-step test: the row of a path (row 0 at step `first`, n live rows) that sits at step s, -1 without one
MRS_TG_HD inline int row_at_step(long long s, int first, int n) {
  MRS_TG_NO_CONTRACT
  const long long r = s - (long long)first;
  return (r >= 0 && r < (long long)n) ? (int)r : -1;
}

// A group's paths [begin, end), clamped into [0, n_paths] with end >= begin: whatever the offsets array holds, no index
// formed from them leaves the plan's arrays.
struct Bounds {
  int begin, end;
};
MRS_TG_HD inline Bounds group_bounds(const int32_t* group_offsets, int g, int n_paths) {
  MRS_TG_NO_CONTRACT
  Bounds b;
  b.begin = group_offsets[g], b.end = group_offsets[g + 1];
  b.begin = b.begin < 0 ? 0 : (b.begin > n_paths ? n_paths : b.begin);
  b.end = b.end < 0 ? 0 : (b.end > n_paths ? n_paths : b.end);
  if (b.end < b.begin) b.end = b.begin;
  return b;
}
// The group of path p: the last g in [0, n_groups) with group_offsets[g] <= p (a group without paths is never the answer for a
// path behind it), and its bounds -- an empty range where the offsets do not put p inside them (offsets that are not
// well-formed; n_groups == 0).  Reads group_offsets[0 .. n_groups] only.
MRS_TG_HD inline Bounds group_of(const int32_t* group_offsets, int n_groups, int p, int n_paths) {
  MRS_TG_NO_CONTRACT
  Bounds none;
  none.begin = none.end = 0;
  if (n_groups <= 0) return none;
  int lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (group_offsets[mid] <= p) lo = mid;
    else hi = mid;
  }
  const Bounds b = group_bounds(group_offsets, lo, n_paths);
  return (p >= b.begin && p < b.end) ? b : none;
}

// the distance of two rows (x, y, z; whatever follows is not read)
MRS_TG_HD inline double distance(const double* a, const double* b, double z_scale) {
  MRS_TG_NO_CONTRACT
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = z_scale * (a[2] - b[2]);
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// The running minimum with its tie rule.  take: the next candidate in increasing index.  better: whether (c, index) comes in
// front of (c2, index2) in the order "smaller value, then lower index" -- the order take realises when it sees the candidates
// one after the other, so minima over parts of the candidates may be combined in any order without changing a bit.
struct Nearest {
  double c;
  int index;  // -1: none
};
MRS_TG_HD inline Nearest nearest_none() {
  MRS_TG_NO_CONTRACT
  Nearest m;
  m.c = no_clearance(), m.index = -1;
  return m;
}
MRS_TG_HD inline void take(Nearest& m, double c, int index) {
  MRS_TG_NO_CONTRACT
  if (c < m.c) m.c = c, m.index = index;
}
MRS_TG_HD inline bool better(double c, int index, double c2, int index2) {
  MRS_TG_NO_CONTRACT
  return c < c2 || (c == c2 && index >= 0 && (index2 < 0 || index < index2));
}

// whether the partner entry of a row of path p names a path of p's group other than p (the caller then asks row_at_step
// whether that path has a live row at the step; only then is anything of it read)
MRS_TG_HD inline bool partner_in_group(int partner, int p, const Bounds& b) {
  MRS_TG_NO_CONTRACT
  return partner >= b.begin && partner < b.end && partner != p;
}

// g dc/drow_i for d = ri - rj: exactly 0 for g == 0 and for coincident rows
MRS_TG_HD inline void row_vjp(const double* ri, const double* rj, double z_scale, double g, double (&gi)[3]) {
  MRS_TG_NO_CONTRACT
  gi[0] = gi[1] = gi[2] = 0.0;
  if (g == 0.0) return;
  const double dx = ri[0] - rj[0], dy = ri[1] - rj[1], dz = z_scale * (ri[2] - rj[2]);
  const double c = sqrt((dx * dx + dy * dy) + dz * dz);
  if (c == 0.0) return;
  gi[0] = g * (dx / c);
  gi[1] = g * (dy / c);
  gi[2] = g * ((z_scale * dz) / c);
}
// g dc/drow_j of the same pair, from row_vjp's result
MRS_TG_HD inline void partner_row(const double (&gi)[3], double (&gj)[3]) {
  MRS_TG_NO_CONTRACT
  for (int k = 0; k < 3; ++k) gj[k] = 0.0 - gi[k];
}

}  // namespace clrq
}  // namespace mrs_tg

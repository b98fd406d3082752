// mrs_tg_obstacle.hpp -- the clearance of every row from a static map of obstacles (mrs_tg_plan_obstacle_clearance,
// obstacle_clearance_kernel) and its backward pass (mrs_tg_plan_obstacle_clearance_vjp, obstacle_clearance_vjp_kernel); DESIGN.md
// section 11j.  An obstacle is four doubles (x, y, z, radius); a radius of 0 is a point of a cloud.  The obstacles live in one
// array obstacles [n_obstacles][4], partitioned into SETS, contiguous runs given by set_offsets [n_sets + 1]; path_set [n_paths]
// names the set a path sees (null: every path sees set 0).  A path sees no obstacle when its path_set entry is outside
// [0, n_sets), when its set is empty or when it is dead.  For a live row (x, y, z) of path p and obstacle k of p's set
//   dx = x - ox,  dy = y - oy,  dz = kappa (z - oz),  s = sqrt((dx dx + dy dy) + dz dz),  c = s - radius,   kappa = z_scale
// (c is signed: negative inside a sphere), and the row's clearance is the minimum of c over k, taken with a strict < from +inf
// in increasing k: a tie goes to the lowest obstacle index, a c that is not a number never becomes a minimum.  nearest = the k
// that gave it, as an index into the WHOLE obstacles array, -1 exactly where the clearance is +inf.  No product is contracted
// into a fused multiply-add, so the CPU and the GPU produce the same bits.  Plain double, __host__ __device__, on mrs_tg_hd.hpp
// alone (through mrs_tg_clearance.hpp, whose running minimum, tie rule, live rows and clamped bounds are used as they are):
// tests/host/obstacle_harness.cpp runs this file under g++.
//
// Backward, the nearest obstacle held fixed.  With g = dL/dclearance of a row, k its nearest and dx, dy, dz, s as above:
//   dL/drow = (g (dx / s), g (dy / s), g ((kappa dz) / s))        row_vjp: each quotient rounded, then the product
// and column 3 (the heading) zero.  g == 0 (so the +inf rows never make a NaN), s == 0 (a row on a centre), a nearest entry
// that is -1 or outside the path's own clamped set contribute exactly 0, and the obstacle is never dereferenced (row_gradient).
//
// Set bounds are clamped into [0, n_obstacles] with end >= begin (clrq::group_bounds), so no index formed from the caller's
// arrays leaves the obstacle array.
//
// Out of scope.  No gradient with respect to the obstacles: they are a static map.  No gradient flows through the choice of
// the obstacle.  A spatial index over the obstacles: for a static map that is mrs_tg_field.hpp's voxel grid.  (The kernel
// spares the square root of obstacles that cannot win, by cannot_win below, which holds the argument why that changes no bit; the plain loop nearest_obstacle is the definition
// and what the harness runs.)
#pragma once

#include "mrs_tg_clearance.hpp"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace obsq {

using clrq::better;
using clrq::Bounds;
using clrq::live_rows;
using clrq::Nearest;
using clrq::nearest_none;
using clrq::no_clearance;
using clrq::take;

// The obstacles [begin, end) path p sees: its set's run clamped into [0, n_obstacles], empty where path_set (null: set 0) names
// no set.  Reads path_set[p] and set_offsets[set], set_offsets[set + 1] only, and those only for a set in [0, n_sets).
MRS_TG_HD inline Bounds path_obstacles(const int32_t* set_offsets, int n_sets, const int32_t* path_set, int p, int n_obstacles) {
  MRS_TG_NO_CONTRACT
  Bounds none;
  none.begin = none.end = 0;
  const int set = path_set ? path_set[p] : 0;
  if (set < 0 || set >= n_sets) return none;
  return clrq::group_bounds(set_offsets, set, n_obstacles);
}

// c of a row (x, y, z; whatever follows is not read) and an obstacle (x, y, z, radius), in its two halves: q, the sum under the
// root, and c from q
MRS_TG_HD inline double distance_squared(const double* row, const double* ob, double z_scale) {
  MRS_TG_NO_CONTRACT
  const double dx = row[0] - ob[0], dy = row[1] - ob[1], dz = z_scale * (row[2] - ob[2]);
  return (dx * dx + dy * dy) + dz * dz;
}
MRS_TG_HD inline double clearance_from(double q, double radius) {
  MRS_TG_NO_CONTRACT
  const double s = sqrt(q);
  return s - radius;
}
MRS_TG_HD inline double clearance(const double* row, const double* ob, double z_scale) {
  MRS_TG_NO_CONTRACT
  return clearance_from(distance_squared(row, ob, z_scale), ob[3]);
}

// THE TEST THAT SPARES A SQUARE ROOT.  true only where c = clearance_from(q, radius) < best is impossible, so that the kernel may
// leave the obstacle out without changing a bit of what the plain loop (nearest_obstacle) gives; false whenever in doubt.
//   t = fl(best + radius);   cannot win  <=  t <= 0,  or  t > 2^-500  and  q > fl(fl(t t) (1 + 2^-20))
// The argument, with eps = 2^-52 and every fl one rounding of relative size at most eps.
// t <= 0 (the row is inside a sphere, or on it, deeper than this obstacle's radius reaches: without this half a single such row
// keeps its whole wavefront taking roots).  t is not a NaN.  t = -inf: best = -inf, below which nothing is, or radius = -inf,
// where c is +inf or a NaN.  Else best and radius are finite and their exact sum is <= 0 (a positive sum rounds to a positive
// value), so best <= -radius; s = fl(sqrt(q)) is >= 0 or a NaN, so s - radius >= -radius >= best in exact arithmetic, and
// rounding is monotone: c >= best or c is a NaN, and c < best is false.
// t > 2^-500.  t is finite or +inf and is
// not a NaN; with t = +inf or t t overflowing the right side is +inf and the test says false, so t t is finite, and above
// 2^-1000 it is a normal number: fl(fl(t t) (1 + 2^-20)) >= t^2 (1 + 2^-20) (1 - eps)^2.  q is above that, so q is not a NaN and
// s = fl(sqrt(q)), correctly rounded, is at least sqrt(q) (1 - eps) > t sqrt(1 + 2^-20) (1 - eps)^2 > t (1 + 2^-23) (s = +inf
// included).  t > 0 is finite, so best and radius are finite and their exact sum e is positive (a sum that is <= 0 rounds to
// a value <= 0), and t >= e (1 - eps).  So s > e (1 - eps) (1 + 2^-23) > e = best + radius, that is s - radius > best in exact
// arithmetic; rounding is monotone and best is a double, so c = fl(s - radius) >= best: c < best is false, take() does nothing.
// `best` may be an OLDER value of the running minimum than the one take() would compare with: the minimum only falls, so
// c >= older best >= best.  The margin 2^-20 is a million times what the proof needs (a few eps); its price is a root taken in
// vain for an obstacle within a millionth of the best one's distance.
MRS_TG_HD inline bool cannot_win(double q, double best, double radius) {
  MRS_TG_NO_CONTRACT
  const double t = best + radius;
  return (t <= 0.0) | ((t > 0x1p-500) & (q > (t * t) * (1.0 + 0x1p-20)));  // (| and &: three compares, no branch)
}

// the row's minimum over the obstacles [b.begin, b.end) in increasing index
MRS_TG_HD inline Nearest nearest_obstacle(const double* row, const double* obstacles, const Bounds& b, double z_scale) {
  MRS_TG_NO_CONTRACT
  Nearest m = nearest_none();
  for (int k = b.begin; k < b.end; ++k) take(m, clearance(row, obstacles + (size_t)k * 4, z_scale), k);
  return m;
}

// whether a nearest entry names an obstacle of the path's own clamped set (only then is it dereferenced)
MRS_TG_HD inline bool nearest_in_set(int nearest, const Bounds& b) {
  MRS_TG_NO_CONTRACT
  return nearest >= b.begin && nearest < b.end;
}

// g dc/drow against one obstacle: exactly 0 for g == 0 and for a row on the centre
MRS_TG_HD inline void row_vjp(const double* row, const double* ob, double z_scale, double g, double (&gi)[3]) {
  MRS_TG_NO_CONTRACT
  gi[0] = gi[1] = gi[2] = 0.0;
  if (g == 0.0) return;
  const double dx = row[0] - ob[0], dy = row[1] - ob[1], dz = z_scale * (row[2] - ob[2]);
  const double s = sqrt((dx * dx + dy * dy) + dz * dz);
  if (s == 0.0) return;
  gi[0] = g * (dx / s);
  gi[1] = g * (dy / s);
  gi[2] = g * ((z_scale * dz) / s);
}

// dL/drow of a live row from its upstream g and its nearest entry: what obstacle_clearance_vjp_kernel writes (with a 0 behind)
MRS_TG_HD inline void row_gradient(const double* row, const double* obstacles, const Bounds& b, int nearest, double z_scale,
                                   double g, double (&gi)[3]) {
  MRS_TG_NO_CONTRACT
  gi[0] = gi[1] = gi[2] = 0.0;
  if (g == 0.0 || !nearest_in_set(nearest, b)) return;
  row_vjp(row, obstacles + (size_t)nearest * 4, z_scale, g, gi);
}

}  // namespace obsq
}  // namespace mrs_tg

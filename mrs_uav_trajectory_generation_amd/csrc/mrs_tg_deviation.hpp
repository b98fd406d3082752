// mrs_tg_deviation.hpp -- the deviation of a sampled trajectory from its waypoint polyline (mrs_tg_plan_path_deviation,
// path_deviation_kernel) and its backward pass (mrs_tg_plan_path_deviation_vjp, path_deviation_vjp_kernel); DESIGN.md
// section 11b.  The scan is validateTrajectorySpatial (mrs_trajectory_generation.cpp:1401-1455 of the reference) with its
// waypoint cursor c: for the samples i = 0 .. n-2 of a path with the waypoints w_0 .. w_S
//   d_i     = dist(s_i, w_c, w_{c+1})          the deviation of sample i, c = c_i
//   e_i     = dist(w_{c+1}, s_i, s_{i+1})      how close the step to the next sample comes to the next waypoint
//   c_{i+1} = c_i + 1 if e_i < 0.05 and c_i < S - 1, else c_i;   c_0 = 0
// dist is distFromSegment (:1533-1554) in the reference's operations and their order (the oracle's mto_dist_from_segment); it
// is the only copy: the policy layer's host code and policy_validate_kernel call it, and validate() below is their scan.  No
// product is contracted into a fused multiply-add, so the CPU and the GPU produce the same bits.  Plain double, __host__ __device__: tests/host/deviation_harness.cpp runs this file under g++.
//
// Backward, cursors and branches held fixed.  With p = s_i, a = w_c, b = w_{c+1}, d = d_i, g = dL/dd_i:
//   coord < 0      dd/dp = (p - a)/d,  dd/da = -dd/dp,           dd/db = 0
//   coord > len    dd/dp = (p - b)/d,  dd/da = 0,                dd/db = -dd/dp
//   interior       dd/dp = u = e/d,    dd/da = -(1 - tau) u,     dd/db = -tau u,    tau = coord/len (0 when len == 0)
// where e is the perpendicular component the forward forms.  d == 0 and g == 0 contribute exactly 0.  Nothing flows through
// s_{i+1}: the advance test is piecewise constant.  THE ORDER OF THE SUMS: every waypoint has one accumulator per coordinate;
// it starts at 0.0 and takes, in increasing sample index, the b-part of the samples whose cursor is w - 1 and then the a-part
// of the samples whose cursor is w (cursors never decrease, so that is increasing sample index throughout).
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace devq {

using mrs_tg::accumulate;

constexpr double kAdvanceDistance = 0.05;  // :1448, a constant of the reference

// What distFromSegment (:1533-1554) forms before it branches, for p against the segment s1 -> s2 (x, y, z; whatever follows is
// not read): the two difference vectors, the segment's length, its direction and the place of p's foot point along it.  dist,
// dist_vjp and passq::fraction (mrs_tg_passage.hpp) all start from this one text.
struct Foot {
  double sv[3], d[3];  // s2 - s1, p - s1
  double n[3];         // sv / len where len * len > 0, else sv
  double len, coord;   // |sv|, n . d
};
MRS_TG_HD inline double norm3(const double (&v)[3]) {
  MRS_TG_NO_CONTRACT
  return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
}
MRS_TG_HD inline Foot foot(const double* p, const double* s1, const double* s2) {
  MRS_TG_NO_CONTRACT
  Foot f;
  for (int k = 0; k < 3; ++k) f.n[k] = f.sv[k] = s2[k] - s1[k];
  f.len = norm3(f.sv);
  if (f.len * f.len > 0)
    for (int k = 0; k < 3; ++k) f.n[k] /= f.len;
  for (int k = 0; k < 3; ++k) f.d[k] = p[k] - s1[k];
  f.coord = f.n[0] * f.d[0] + f.n[1] * f.d[1] + f.n[2] * f.d[2];
  return f;
}

// distFromSegment (:1533-1554): the distance of p from the segment s1 -> s2
MRS_TG_HD inline double dist(const double* p, const double* s1, const double* s2) {
  MRS_TG_NO_CONTRACT
  const Foot f = foot(p, s1, s2);
  if (f.coord < 0) return norm3(f.d);
  if (f.coord > f.len) {
    const double e[3] = {p[0] - s2[0], p[1] - s2[1], p[2] - s2[2]};
    return norm3(e);
  }
  const double e[3] = {p[0] - (s1[0] + f.n[0] * f.coord), p[1] - (s1[1] + f.n[1] * f.coord), p[2] - (s1[2] + f.n[2] * f.coord)};
  return norm3(e);
}

// whether the cursor c of a path with S segments moves on behind sample s (next: the sample after it)
MRS_TG_HD inline bool advances(const double* next_waypoint, const double* s, const double* next, int c, int S) {
  return dist(next_waypoint, s, next) < kAdvanceDistance && c < S - 1;
}

// whether sample i counts towards the maxima (:1437)
MRS_TG_HD inline bool counted(int c, int first_segment, int S) { return c > 0 || first_segment != 0 || S + 1 <= 2; }

// validateTrajectorySpatial (:1401-1455) for one path, one sample after the other: samples [n][4], waypoints [n_wp][4] (x, y, z
// are read).  safe [n_wp - 1] is written in full: 0 where a counted sample of the segment strays further than max_deviation.
struct Validation {
  bool is_safe;
  double max_deviation;  // of the counted samples
};
MRS_TG_HD inline Validation validate(const double* samples, int n, const double* waypoints, int n_wp, int first_segment,
                                     double max_deviation, uint8_t* safe) {
  const int S = n_wp - 1;
  Validation v;
  v.is_safe = true, v.max_deviation = 0.0;
  for (int i = 0; i < S; ++i) safe[i] = 1;
  int c = 0;
  for (int i = 0; i + 1 < n && S >= 1; ++i) {
    const double* s = samples + (size_t)i * 4;
    const double* a = waypoints + (size_t)c * 4;
    const double d = dist(s, a, a + 4);
    const bool moves_on = advances(a + 4, s, s + 4, c, S);  // (in front of the store to safe[], which may alias the rows)
    if (counted(c, first_segment, S)) {
      if (d > v.max_deviation) v.max_deviation = d;
      if (d > max_deviation) safe[c] = 0, v.is_safe = false;
    }
    if (moves_on) ++c;
  }
  return v;
}

// g * dd/dp, g * dd/da, g * dd/db of d = dist(p, a, b), the branch being the forward's
MRS_TG_HD inline void dist_vjp(const double* p, const double* a, const double* b, double g, double (&gp)[3], double (&ga)[3],
                               double (&gb)[3]) {
  MRS_TG_NO_CONTRACT
  for (int k = 0; k < 3; ++k) gp[k] = ga[k] = gb[k] = 0.0;
  if (g == 0.0) return;
  const Foot f = foot(p, a, b);
  if (f.coord < 0) {
    const double d = norm3(f.d);
    if (d == 0.0) return;
    for (int k = 0; k < 3; ++k) gp[k] = g * (f.d[k] / d);
    for (int k = 0; k < 3; ++k) ga[k] = 0.0 - gp[k];
    return;
  }
  if (f.coord > f.len) {
    const double e[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
    const double d = norm3(e);
    if (d == 0.0) return;
    for (int k = 0; k < 3; ++k) gp[k] = g * (e[k] / d);
    for (int k = 0; k < 3; ++k) gb[k] = 0.0 - gp[k];
    return;
  }
  const double e[3] = {p[0] - (a[0] + f.n[0] * f.coord), p[1] - (a[1] + f.n[1] * f.coord), p[2] - (a[2] + f.n[2] * f.coord)};
  const double d = norm3(e);
  if (d == 0.0) return;
  const double tau = f.len * f.len > 0 ? f.coord / f.len : 0.0;
  const double rest = 1.0 - tau;
  for (int k = 0; k < 3; ++k) gp[k] = g * (e[k] / d);
  for (int k = 0; k < 3; ++k) {
    ga[k] = 0.0 - rest * gp[k];
    gb[k] = 0.0 - tau * gp[k];
  }
}

}  // namespace devq
}  // namespace mrs_tg

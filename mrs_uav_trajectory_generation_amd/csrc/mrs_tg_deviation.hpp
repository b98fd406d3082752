// mrs_tg_deviation.hpp -- the deviation of a sampled trajectory from its waypoint polyline (mrs_tg_plan_path_deviation,
// path_deviation_kernel) and its backward pass (mrs_tg_plan_path_deviation_vjp, path_deviation_vjp_kernel); DESIGN.md
// section 11b.  The scan is validateTrajectorySpatial (mrs_trajectory_generation.cpp:1401-1455 of the reference) with its
// waypoint cursor c: for the samples i = 0 .. n-2 of a path with the waypoints w_0 .. w_S
//   d_i     = dist(s_i, w_c, w_{c+1})          the deviation of sample i, c = c_i
//   e_i     = dist(w_{c+1}, s_i, s_{i+1})      how close the step to the next sample comes to the next waypoint
//   c_{i+1} = c_i + 1 if e_i < 0.05 and c_i < S - 1, else c_i;   c_0 = 0
// dist is distFromSegment (:1533-1554) with the host's operations in the host's order (mrs_tg_policy_host.hpp's
// dist_from_segment, the oracle's mto_dist_from_segment): no product is contracted into a fused multiply-add, so the CPU and
// the GPU produce the same bits.  Plain double, __host__ __device__: tests/host/deviation_harness.cpp runs this file under g++.
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

// distFromSegment (:1533-1554): the distance of p from the segment s1 -> s2 (x, y, z; whatever follows is not read)
MRS_TG_HD inline double dist(const double* p, const double* s1, const double* s2) {
  MRS_TG_NO_CONTRACT
  const double sv0 = s2[0] - s1[0], sv1 = s2[1] - s1[1], sv2 = s2[2] - s1[2];
  const double len = sqrt(sv0 * sv0 + sv1 * sv1 + sv2 * sv2);
  double n0 = sv0, n1 = sv1, n2 = sv2;
  if (len * len > 0) {
    n0 /= len;
    n1 /= len;
    n2 /= len;
  }
  const double d0 = p[0] - s1[0], d1 = p[1] - s1[1], d2 = p[2] - s1[2];
  const double coord = n0 * d0 + n1 * d1 + n2 * d2;
  if (coord < 0) return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  if (coord > len) {
    const double e0 = p[0] - s2[0], e1 = p[1] - s2[1], e2 = p[2] - s2[2];
    return sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  }
  const double f0 = p[0] - (s1[0] + n0 * coord), f1 = p[1] - (s1[1] + n1 * coord), f2 = p[2] - (s1[2] + n2 * coord);
  return sqrt(f0 * f0 + f1 * f1 + f2 * f2);
}

// whether the cursor c of a path with S segments moves on behind sample s (next: the sample after it)
MRS_TG_HD inline bool advances(const double* next_waypoint, const double* s, const double* next, int c, int S) {
  return dist(next_waypoint, s, next) < kAdvanceDistance && c < S - 1;
}

// whether sample i counts towards the maxima (:1437)
MRS_TG_HD inline bool counted(int c, int first_segment, int S) { return c > 0 || first_segment != 0 || S + 1 <= 2; }

// g * dd/dp, g * dd/da, g * dd/db of d = dist(p, a, b), the branch being the forward's
MRS_TG_HD inline void dist_vjp(const double* p, const double* a, const double* b, double g, double (&gp)[3], double (&ga)[3],
                               double (&gb)[3]) {
  MRS_TG_NO_CONTRACT
  for (int k = 0; k < 3; ++k) gp[k] = ga[k] = gb[k] = 0.0;
  if (g == 0.0) return;
  const double sv0 = b[0] - a[0], sv1 = b[1] - a[1], sv2 = b[2] - a[2];
  const double len = sqrt(sv0 * sv0 + sv1 * sv1 + sv2 * sv2);
  double n0 = sv0, n1 = sv1, n2 = sv2;
  if (len * len > 0) {
    n0 /= len;
    n1 /= len;
    n2 /= len;
  }
  const double d0 = p[0] - a[0], d1 = p[1] - a[1], d2 = p[2] - a[2];
  const double coord = n0 * d0 + n1 * d1 + n2 * d2;
  if (coord < 0) {
    const double d = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    if (d == 0.0) return;
    gp[0] = g * (d0 / d), gp[1] = g * (d1 / d), gp[2] = g * (d2 / d);
    for (int k = 0; k < 3; ++k) ga[k] = 0.0 - gp[k];
    return;
  }
  if (coord > len) {
    const double e0 = p[0] - b[0], e1 = p[1] - b[1], e2 = p[2] - b[2];
    const double d = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    if (d == 0.0) return;
    gp[0] = g * (e0 / d), gp[1] = g * (e1 / d), gp[2] = g * (e2 / d);
    for (int k = 0; k < 3; ++k) gb[k] = 0.0 - gp[k];
    return;
  }
  const double f0 = p[0] - (a[0] + n0 * coord), f1 = p[1] - (a[1] + n1 * coord), f2 = p[2] - (a[2] + n2 * coord);
  const double d = sqrt(f0 * f0 + f1 * f1 + f2 * f2);
  if (d == 0.0) return;
  const double tau = len * len > 0 ? coord / len : 0.0;
  const double rest = 1.0 - tau;
  gp[0] = g * (f0 / d), gp[1] = g * (f1 / d), gp[2] = g * (f2 / d);
  for (int k = 0; k < 3; ++k) {
    ga[k] = 0.0 - rest * gp[k];
    gb[k] = 0.0 - tau * gp[k];
  }
}

}  // namespace devq
}  // namespace mrs_tg

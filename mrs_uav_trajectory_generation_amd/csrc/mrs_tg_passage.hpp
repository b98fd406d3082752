// mrs_tg_passage.hpp -- where a sampled trajectory passes the requested waypoints (mrs_tg_plan_waypoint_passage,
// waypoint_passage_kernel) and its backward pass (mrs_tg_plan_waypoint_passage_vjp, waypoint_passage_vjp_kernel); DESIGN.md
// section 11c.  The scan is getWaypointInTrajectoryIdxs (mrs_trajectory_generation.cpp:1461-1499 of the reference) with its
// waypoint cursor c: for the steps i = 0 .. n-2 of a path with the waypoints w_0 .. w_{W-1}, c = 0 at the start,
//   m = dist(w_c, s_i, s_{i+1});   if m < 0.1:  index[c] = i, miss[c] = m, fraction[c] = tau, c = c + 1;   stop when c == W
// dist is devq::dist of mrs_tg_deviation.hpp, unchanged.  tau is the place of the foot point on the step, from the very coord
// and len that dist forms (devq::foot): 0 when coord < 0 or len * len == 0, 1 when coord > len, otherwise coord / len.  A
// distance that is not a number is no hit.  Plain double, __host__ __device__, no product contracted into a fused multiply-add:
// tests/host/passage_harness.cpp runs this file under g++ and the kernels give its bits.
//
// Backward, indices and branches held fixed.  For a hit of p = w_k on the step a = s_i, b = s_{i+1} with the upstreams
// g_m = dL/dmiss[k], g_t = dL/dfraction[k]: the miss part is devq::dist_vjp(p, a, b, g_m) as it stands; the fraction part is
// zero in the two clamped branches and for len * len == 0, and in the interior, with v = b - a, q = p - a, L2 = len * len,
//   dtau/dp = v / L2,   dtau/db = (q - 2 tau v) / L2,   dtau/da = -dtau/dp - dtau/db
// in THIS ORDER OF OPERATIONS per coordinate k (v_k, q_k, len, coord as dist forms them):
//   L2 = len * len;  tau = coord / len;  t2 = 2.0 * tau;
//   tp_k = v_k / L2;  tb_k = (q_k - t2 * v_k) / L2;  ta_k = (0.0 - tp_k) - tb_k;   g_t * tp_k,  g_t * ta_k,  g_t * tb_k
// coord == 0 and coord == len take the interior row.  m == 0 contributes exactly 0 through the miss, a zero upstream exactly 0.
// THE ORDER OF THE SUMS: a hit's contribution to a row is, per coordinate, accumulate(miss part, fraction part).  A waypoint's
// row is that one term.  Sample row j starts at 0.0 and takes the b-contribution of the hit on step j - 1, if there is one,
// then the a-contribution of the hit on step j, if there is one; a step takes at most one waypoint, so that is the whole sum.
#pragma once

#include "mrs_tg_deviation.hpp"

namespace mrs_tg {
namespace passq {

using mrs_tg::accumulate;

constexpr double kPassDistance = 0.1;  // :1487, a constant of the reference

// tau of the foot point of p on the step a -> b (x, y, z; whatever follows is not read)
MRS_TG_HD inline double fraction(const double* p, const double* a, const double* b) {
  MRS_TG_NO_CONTRACT
  const devq::Foot f = devq::foot(p, a, b);
  if (f.coord < 0 || f.len * f.len == 0) return 0.0;
  if (f.coord > f.len) return 1.0;
  return f.coord / f.len;
}

// g * dtau/dp, g * dtau/da, g * dtau/db of tau = fraction(p, a, b), the branch being the forward's
MRS_TG_HD inline void fraction_vjp(const double* p, const double* a, const double* b, double g, double (&gp)[3], double (&ga)[3],
                                   double (&gb)[3]) {
  MRS_TG_NO_CONTRACT
  for (int k = 0; k < 3; ++k) gp[k] = ga[k] = gb[k] = 0.0;
  if (g == 0.0) return;
  const devq::Foot f = devq::foot(p, a, b);
  if (f.coord < 0 || f.len * f.len == 0 || f.coord > f.len) return;
  const double L2 = f.len * f.len;
  const double tau = f.coord / f.len;
  const double t2 = 2.0 * tau;
  for (int k = 0; k < 3; ++k) {
    const double tp = f.sv[k] / L2;
    const double tb = (f.d[k] - t2 * f.sv[k]) / L2;
    const double ta = (0.0 - tp) - tb;
    gp[k] = g * tp;
    ga[k] = g * ta;
    gb[k] = g * tb;
  }
}

// the scan's hit test: whether the step a -> b takes the waypoint w; m: its distance from the step (not a number: no hit)
MRS_TG_HD inline bool hit(const double* w, const double* a, const double* b, double& m) {
  m = devq::dist(w, a, b);
  return m < kPassDistance;
}

// The three rows of one hit: the miss part, then + the fraction part, per coordinate
MRS_TG_HD inline void hit_vjp(const double* p, const double* a, const double* b, double g_miss, double g_fraction,
                              double (&gp)[3], double (&ga)[3], double (&gb)[3]) {
  double fp[3], fa[3], fb[3];
  devq::dist_vjp(p, a, b, g_miss, gp, ga, gb);
  fraction_vjp(p, a, b, g_fraction, fp, fa, fb);
  for (int k = 0; k < 3; ++k) {
    gp[k] = accumulate(gp[k], fp[k]);
    ga[k] = accumulate(ga[k], fa[k]);
    gb[k] = accumulate(gb[k], fb[k]);
  }
}

// The scan as the reference writes it, one step after the other: waypoints [W][wstride], samples [n][sstride] (x, y, z first).
// Writes index / miss / fraction [W] in full (-1 / 0.0 / 0.0 from the first waypoint not reached on) and returns the count.
inline int scan(const double* waypoints, int W, int wstride, const double* samples, int n, int sstride, int32_t* index,
                double* miss, double* fraction_out) {
  int c = 0;
  for (int i = 0; i + 1 < n && c < W; ++i) {
    const double* w = waypoints + (size_t)c * wstride;
    const double* a = samples + (size_t)i * sstride;
    double m;
    if (hit(w, a, a + sstride, m)) {
      index[c] = i;
      miss[c] = m;
      fraction_out[c] = fraction(w, a, a + sstride);
      ++c;
    }
  }
  for (int k = c; k < W; ++k) index[k] = -1, miss[k] = 0.0, fraction_out[k] = 0.0;
  return c;
}

// The backward pass over the hits of scan() (index [count]) in the order of the sums stated above: grad_samples [n][3] and
// grad_waypoints [W][3] are written in full.  grad_miss / grad_fraction [W] may be null (zero); entries from count on are
// not read.
inline void scan_vjp(const double* waypoints, int W, int wstride, const double* samples, int n, int sstride, const int32_t* index,
                     int count, const double* grad_miss, const double* grad_fraction, double* grad_samples,
                     double* grad_waypoints) {
  for (size_t e = 0; e < (size_t)(n > 0 ? n : 0) * 3; ++e) grad_samples[e] = 0.0;
  for (size_t e = 0; e < (size_t)W * 3; ++e) grad_waypoints[e] = 0.0;
  for (int k = 0; k < count; ++k) {
    const int i = index[k];
    const double* w = waypoints + (size_t)k * wstride;
    const double* a = samples + (size_t)i * sstride;
    double gp[3], ga[3], gb[3];
    hit_vjp(w, a, a + sstride, grad_miss ? grad_miss[k] : 0.0, grad_fraction ? grad_fraction[k] : 0.0, gp, ga, gb);
    for (int j = 0; j < 3; ++j) {
      grad_waypoints[(size_t)k * 3 + j] = gp[j];
      // (row i has taken the b-contribution of the hit on step i - 1 already, if there was one: the hits come in increasing i)
      grad_samples[(size_t)i * 3 + j] = accumulate(grad_samples[(size_t)i * 3 + j], ga[j]);
      grad_samples[(size_t)(i + 1) * 3 + j] = accumulate(grad_samples[(size_t)(i + 1) * 3 + j], gb[j]);
    }
  }
}

}  // namespace passq
}  // namespace mrs_tg

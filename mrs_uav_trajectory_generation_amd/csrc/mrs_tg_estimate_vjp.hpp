// mrs_tg_estimate_vjp.hpp -- the backward pass of the Euclidean segment-time estimate (mrs_tg_plan_estimate_times_vjp,
// estimate_times_vjp_kernel); DESIGN.md section 4e.  The forward is estimate_segment_time (mrs_tg_estimate.hpp,
// estimateSegmentTimesEuclidean, vertex.cpp:491-565 of the reference) and stays where it is; classify() below is its sibling:
// the same expressions in the same order, contraction off, which also says which TERM the value came from
//   HORIZONTAL  t = h / v_h          |inclination| <= atan2(v_v, v_h)
//   VERTICAL    t = |dz| / v_v       steeper than that
//   FLOOR       t = 0.01             the distance term was below it
//   HEADING     t = 1.5 (t_vel + t_acc) exceeded all of that, strictly
// and what the heading term's own branches were: cruise (the forward's `reduced >= 0`) and acc (ang > pi/4).  Plain double,
// __host__ __device__: tests/host/estimate_vjp_harness.cpp runs this file under g++.
//
// Backward, every branch held fixed.  With G = dL/dt, d = e - s, h = sqrt(dx^2 + dy^2), delta the forward's signed wrapped
// heading difference (start minus end), ang = |delta|, w = lim[2], a = lim[5]:
//   HORIZONTAL  dt/de = (dx/h, dy/h, 0, 0)/v_h            dt/dv_h = -(h/v_h)/v_h
//   VERTICAL    dt/de = (0, 0, sign(dz), 0)/v_v           dt/dv_v = -(|dz|/v_v)/v_v
//   FLOOR       nothing
//   HEADING     dt/de = (0, 0, 0, -1.5 sign(delta)/w)     dt/dw = 1.5 (-ang/w^2 - [cruise] 1/a + [acc] 2/a)
//                                                         dt/da = 1.5 ([cruise] w/a^2 - [acc] 2 w/a^2)
// and dt/ds = -dt/de.  Subtraction, multiplication, division and square root only: no transcendental enters a gradient's value
// (atan2, sin, cos and fmod decide the term, as they decide it in the forward), so the CPU and the GPU produce the same bits.
// G == 0 contributes exactly 0; a segment with a non-finite waypoint or time, or a limit that is not a number, contributes
// zeros and reports FLOOR.  THE ORDER OF THE SUMS: a vertex's accumulator starts at 0.0 and takes the end-part of the segment
// in front of it, then the start-part of its own segment; a path's limit accumulators start at 0.0 and take the path's
// segments in increasing index.
#pragma once

#include <cfloat>

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace estvjp {

using mrs_tg::accumulate;

constexpr int kHorizontal = 0, kVertical = 1, kFloor = 2, kHeading = 3;  // MRS_TG_ESTIMATE_TERM_*
constexpr int kLimits = 9;                                              // limits per path, index 3 (k - 1) + group
constexpr int kVh = 0, kVv = 1, kW = 2, kA = 5;                         // the four the estimate reads
constexpr double kFloorTime = 0.01;
constexpr double kPi = 3.14159265358979323846;                          // M_PI, digit for digit

MRS_TG_HD inline double wrap_pi(double a) {
  MRS_TG_NO_CONTRACT
  const double two_pi = 2.0 * kPi;
  double r = fmod(a + kPi, two_pi);
  if (r < 0) r += two_pi;
  return r - kPi;
}

// the forward's heading difference before its fabs: start minus end, in [-pi, pi)
MRS_TG_HD inline double signed_angle_dist(double a, double bb) {
  MRS_TG_NO_CONTRACT
  const double two_pi = 2.0 * kPi;
  double dlt = wrap_pi(a) - wrap_pi(bb);
  if (dlt < -kPi) dlt += two_pi;
  else if (dlt >= kPi) dlt -= two_pi;
  return dlt;
}

struct Segment {
  int term;
  double value;          // the forward's time
  double dx, dy, dz, h;  // end minus start; h = sqrt(dx^2 + dy^2)
  double delta, ang;     // the signed heading difference and its magnitude
  bool cruise, acc;      // the heading term's branches (false where the heading is relaxed)
};

MRS_TG_HD inline bool finite(double x) { return x - x == 0.0; }

// s: the segment's start waypoint (x, y, z, heading), the end waypoint behind it; lim: the path's nine limits
MRS_TG_HD inline Segment classify(const double* s, const double* lim) {
  MRS_TG_NO_CONTRACT
  const double* e = s + 4;
  const double v_h = lim[kVh], v_v = lim[kVv], w_max = lim[kW], a_max = lim[kA];
  Segment c;
  c.dx = e[0] - s[0], c.dy = e[1] - s[1], c.dz = e[2] - s[2];
  const double dx = c.dx, dy = c.dy, dz = c.dz;
  c.h = sqrt(dx * dx + dy * dy);
  const double inclinator = atan2(dz, sqrt(dx * dx + dy * dy));
  const double thr = atan2(v_v, v_h);
  const bool vertical = inclinator > thr || inclinator < -thr;
  const double vmax = vertical ? fabs(v_v / sin(inclinator)) : fabs(v_h / cos(inclinator));
  double t = sqrt(dx * dx + dy * dy + dz * dz) / vmax;
  const bool floored = t < kFloorTime;
  if (floored) t = kFloorTime;
  c.delta = signed_angle_dist(s[3], e[3]);
  const double ang = fabs(c.delta);
  c.ang = ang;
  c.cruise = c.acc = false;
  double t_vel = 0.0, t_acc = 0.0;
  if (w_max < (double)FLT_MAX && a_max < (double)FLT_MAX) {
    const double reduced = (ang - (w_max * w_max) / a_max) / w_max;
    c.cruise = !(reduced < 0);
    t_vel = (reduced < 0) ? ang / w_max : reduced;
    if (ang > kPi / 4) {
      c.acc = true;
      t_acc = 2 * (w_max / a_max);
    }
  }
  const double hf = 1.5 * (t_vel + t_acc);
  const bool heading = hf > t;  // (a tie stays with the distance term)
  if (heading) t = hf;
  c.value = t;
  c.term = heading ? kHeading : floored ? kFloor : vertical ? kVertical : kHorizontal;
  bool usable = finite(t) && v_h == v_h && v_v == v_v && w_max == w_max && a_max == a_max;
  for (int k = 0; k < 8; ++k) usable = usable && finite(s[k]);
  if (!usable) c.term = kFloor;
  return c;
}

// G dt/de (the end waypoint's row; the start waypoint's is its negative) and G dt/d(v_h, v_v, w, a)
struct Partials {
  double end[4];
  double v_h, v_v, w, a;
};

MRS_TG_HD inline double sign_of(double x) { return x > 0 ? 1.0 : x < 0 ? -1.0 : 0.0; }

MRS_TG_HD inline Partials partials(const Segment& c, const double* lim, double G) {
  MRS_TG_NO_CONTRACT
  Partials p{{0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, 0.0};
  if (G == 0.0) return p;
  if (c.term == kHorizontal) {
    const double v_h = lim[kVh];
    if (c.h == 0.0) return p;  // (coincident waypoints are FLOOR; a purely vertical segment is VERTICAL)
    p.end[0] = G * ((c.dx / c.h) / v_h);
    p.end[1] = G * ((c.dy / c.h) / v_h);
    p.v_h = G * (0.0 - (c.h / v_h) / v_h);
  } else if (c.term == kVertical) {
    const double v_v = lim[kVv];
    p.end[2] = G * (sign_of(c.dz) / v_v);
    p.v_v = G * (0.0 - (fabs(c.dz) / v_v) / v_v);
  } else if (c.term == kHeading) {
    const double w = lim[kW], a = lim[kA];
    p.end[3] = G * (0.0 - 1.5 * (sign_of(c.delta) / w));
    double dw = 0.0 - c.ang / (w * w);
    if (c.cruise) dw = dw - 1.0 / a;
    if (c.acc) dw = dw + 2.0 / a;
    p.w = G * (1.5 * dw);
    const double q = w / (a * a);
    double da = 0.0;
    if (c.cruise) da = da + q;
    if (c.acc) da = da - 2.0 * q;
    p.a = G * (1.5 * da);
  }
  return p;
}

// dL/dwaypoint of one vertex: the end-part of the segment in front of it (front: its start waypoint, or null for a path's
// first vertex; G_front its upstream), then the start-part of its own segment (own: this vertex's waypoint, with the end
// waypoint behind it, or null for a path's last vertex).  term_out: the term of the own segment, may be null.
MRS_TG_HD inline void vertex_gradient(const double* front, double G_front, const double* own, double G_own, const double* lim,
                                      double (&g)[4], int* term_out) {
  for (int k = 0; k < 4; ++k) g[k] = 0.0;
  if (front) {
    const Partials p = partials(classify(front, lim), lim, G_front);
    for (int k = 0; k < 4; ++k) g[k] = accumulate(g[k], p.end[k]);
  }
  if (own) {
    const Segment c = classify(own, lim);
    if (term_out) *term_out = c.term;
    const Partials p = partials(c, lim, G_own);
    for (int k = 0; k < 4; ++k) g[k] = accumulate(g[k], 0.0 - p.end[k]);
  }
}

// dL/dlimits of one path: wp its S + 1 waypoints, G its S upstream entries; entries 3, 4, 6, 7 and 8 stay 0
MRS_TG_HD inline void limit_gradient(const double* wp, const double* G, int S, const double* lim, double (&g)[kLimits]) {
  for (int k = 0; k < kLimits; ++k) g[k] = 0.0;
  for (int j = 0; j < S; ++j) {
    const double* s = wp + (size_t)j * 4;
    const Partials p = partials(classify(s, lim), lim, G[j]);
    g[kVh] = accumulate(g[kVh], p.v_h);
    g[kVv] = accumulate(g[kVv], p.v_v);
    g[kW] = accumulate(g[kW], p.w);
    g[kA] = accumulate(g[kA], p.a);
  }
}

}  // namespace estvjp
}  // namespace mrs_tg

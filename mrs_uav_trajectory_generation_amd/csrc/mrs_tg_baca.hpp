// mrs_tg_baca.hpp -- the Baca segment-time estimate as a plan step, its backward pass and the length gate
// (mrs_tg_plan_estimate_times_baca, mrs_tg_plan_estimate_times_baca_vjp, mrs_tg_plan_length_gate; baca_times_kernel,
// baca_times_vjp_kernel, length_gate_kernel).  The forward is estimateSegmentTimesBaca
// (vertex.cpp:301-485 of the reference), operation by operation, contraction off; classify() below IS that forward -- the
// kernel's value and the host's policy::estimate_times_baca (mrs_tg_policy_host.hpp) are both classify().value -- and beside
// the value it says which branches were taken (MRS_TG_BACA_*):
//   V_VERTICAL, A_VERTICAL, J_VERTICAL   |inclination| > atan2(L_v, L_h), decided separately for L = v, a, j
//   T1_CAPPED, T2_CAPPED                 sqrt(2 distance / a_max) was the smaller (t > cap, strictly)
//   DOT1_CLAMPED, DOT2_CLAMPED           the corner's cosine was negative (dot < 0, strictly): the coefficient is the constant 1
//   FLOOR                                t < 0.01, strictly: the forward took 0.01
//   HEADING                              1.5 (t_vel + t_acc) exceeded all of that, strictly
//   HEADING_CRUISE, HEADING_ACC          the heading term's branches: the forward's `reduced >= 0`, and ang > pi/4
// A segment's neighbours are those of its own path: segment 0 takes the full acceleration time in front, segment S - 1 behind.
// Plain double, __host__ __device__ (section 4a): tests/host/baca_harness.cpp runs this file under g++.  The value is NOT
// promised in the host's bits: atan2, sin and cos are the device's.
//
// Backward, every branch held fixed.  G = dL/dt, pre, s, e, post the four waypoints, d = e - s, D = |d|, h = sqrt(dx^2 + dy^2);
// for L in {v, a, j}: c_L = L_h, q_L = h (horizontal regime) or c_L = L_v, q_L = |dz| (vertical regime), and
//   L_max = c_L D / q_L        (the forward's |L_h / cos| or |L_v / sin| up to roundings)
//   grad q = (dx/h, dy/h, 0) or (0, 0, sign dz)   rho_L = grad q_L / q_L
//   full = v_max/a_max + a_max/j_max              dfull/de = (v_max/a_max)(rho_a - rho_v) + (a_max/j_max)(rho_j - rho_a)
//   cap = sqrt(2 D / a_max)                       dcap/de = cap rho_a / 2            dcap/dc_a = -(cap/2)/c_a
//   u1 = (s - pre)/n1, u2 = d/D, u3 = (post - e)/n3 (the forward's unit vectors), dot1 = u1.u2, dot2 = u2.u3
//   c1 = 1 (segment 0, or DOT1_CLAMPED) or 1 - dot1;  c2 = 1 (segment S - 1, or DOT2_CLAMPED) or 1 - dot2
//   t = D/v_max + t1 + t2,  t_i = c_i full, or cap where T_i_CAPPED
//   D/v_max = q_v/c_v:   d/de = grad q_v / c_v                          d/dc_v = -(q_v/c_v)/c_v
//   t_i = c_i full:      d/de = c_i dfull/de + full dc_i/de             d/dc_v = c_i (v_max/a_max)/c_v
//                        d/dc_a = -c_i (v_max/a_max)/c_a + c_i (a_max/j_max)/c_a       d/dc_j = -c_i (a_max/j_max)/c_j
//   c1 = 1 - dot1:       dc1/dpre = (u2 - dot1 u1)/n1    dc1/ds = -(u2 - dot1 u1)/n1 + (u1 - dot1 u2)/D    dc1/de = -(u1 - dot1 u2)/D
//   c2 = 1 - dot2:       dc2/ds = (u3 - dot2 u2)/D       dc2/de = -(u3 - dot2 u2)/D + (u2 - dot2 u3)/n3    dc2/dpost = -(u2 - dot2 u3)/n3
//   and d/ds = -d/de for D/v_max, full and cap.
//   FLOOR    nothing
//   HEADING  dt/de = (0, 0, 0, -1.5 sign(delta)/w), dt/ds its negative, delta the forward's signed wrapped heading difference
//            (start minus end), ang = |delta|, w = lim[2], a = lim[5]:
//            dt/dw = 1.5 (-ang/w^2 - [cruise] 2/a + [acc] 2/a)      dt/da = 1.5 ([cruise] 2 w/a^2 - [acc] 2 w/a^2)
//            (the row of section 4e with the reference's `2 *` in front of w^2/a in this estimator's cruise branch)
// Subtraction, multiplication, division and square root only: no transcendental enters a gradient's value, so the CPU and the
// GPU produce the same bits.  A zero-length neighbour has the zero unit vector, as in the forward, and gives no gradient
// through it.  G == 0 contributes exactly 0; a segment with a non-finite waypoint, time or limit contributes zeros and reports
// flags = FLOOR.  Limit entry 8 is never touched.  THE ORDER OF THE SUMS: inside a segment every part is the sum, from 0.0, of
// its addends in the order partials() lists them, times G; a vertex's accumulator starts at 0.0 and takes, of the segments that
// exist, the post-part of segment v - 2, the end-part of v - 1, the start-part of v, the pre-part of v + 1; a path's limit
// accumulators start at 0.0 and take the path's segments in increasing index.
#pragma once

#include <cfloat>

#include "mrs_tg_estimate_vjp.hpp"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace baca {

using estvjp::finite;
using estvjp::kFloorTime;
using estvjp::kLimits;
using estvjp::kPi;
using estvjp::sign_of;
using mrs_tg::accumulate;

constexpr int kVVertical = 1, kAVertical = 2, kJVertical = 4, kT1Capped = 8, kT2Capped = 16, kDot1Clamped = 32,
              kDot2Clamped = 64, kFloor = 128, kHeading = 256, kHeadingCruise = 512, kHeadingAcc = 1024;  // MRS_TG_BACA_*
constexpr int kVerdictAccepted = 0, kVerdictCode = 1, kVerdictTooLong = 2, kVerdictTooShort = 3;           // MRS_TG_FIND_*

// mrs_lib's wrap and radians::diff (angles into [0, 2 pi)); the policy layer's heading unwrap and interpolation use them too
MRS_TG_HD inline double wrap_range(double a, double lo, double range) {
  MRS_TG_NO_CONTRACT
  double r = fmod(a - lo, range);
  if (r < 0) r += range;
  return r + lo;
}
MRS_TG_HD inline double radians_diff(double minuend, double subtrahend) {
  MRS_TG_NO_CONTRACT
  const double two_pi = 2.0 * kPi;
  double d = wrap_range(minuend, 0.0, two_pi) - wrap_range(subtrahend, 0.0, two_pi);
  if (d < -kPi) d += two_pi;
  else if (d >= kPi) d -= two_pi;
  return d;
}

// vertex.cpp:337-353, one of v, a, j
struct Limit {
  bool vertical;
  double thr, value;
};
// the three atan2(L_v, L_h) of a path, L = v, a, j: the same for every segment of it, so a lane that takes several computes them once
struct Thresholds {
  double thr[3];
};
MRS_TG_HD inline Thresholds thresholds(const double* lim) {
  Thresholds t;
  t.thr[0] = atan2(lim[1], lim[0]), t.thr[1] = atan2(lim[4], lim[3]), t.thr[2] = atan2(lim[7], lim[6]);
  return t;
}
MRS_TG_HD inline Limit limit_for_inclination(double inclinator, double lim_v, double lim_h, double thr) {
  MRS_TG_NO_CONTRACT
  Limit L;
  L.thr = thr;
  L.vertical = inclinator > L.thr || inclinator < -L.thr;
  L.value = L.vertical ? fabs(lim_v / sin(inclinator)) : fabs(lim_h / cos(inclinator));
  return L;
}

// (b - a) normalised where its squared norm is positive, as Eigen's normalize(); -> the norm
MRS_TG_HD inline double unit3(const double* a, const double* b, double* u) {
  MRS_TG_NO_CONTRACT
  double v[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (n * n > 0) {
    v[0] /= n;
    v[1] /= n;
    v[2] /= n;
  }
  u[0] = v[0], u[1] = v[1], u[2] = v[2];
  return n;
}

MRS_TG_HD inline double dot3(const double* a, const double* b) {
  MRS_TG_NO_CONTRACT
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

struct Segment {
  int flags;
  double value;                 // the forward's time
  bool has_pre, has_post;       // a corner in front (i >= 1) and behind (i < S - 1)
  double d[3], D, h;            // end minus start, its length, its horizontal length
  double u1[3], u2[3], u3[3];   // the forward's unit vectors pre -> s, s -> e, e -> post
  double n1, n3, dot1, dot2;
  double delta, ang;            // the signed heading difference (start minus end) and its magnitude
  // what the harness reads the distance to the branch boundaries from
  double inclinator, thr[3], t1_raw, t2_raw, cap, t_dist, hf, ang_cruise;
  bool relaxed;
};

// wp: the path's first waypoint row (x, y, z, heading); i: the segment within its path, 0 .. S - 1; lim: the path's nine limits,
// th: thresholds(lim)
MRS_TG_HD inline Segment classify(const double* wp, int i, int S, const double* lim, const Thresholds& th) {
  MRS_TG_NO_CONTRACT
  const double v_h = lim[0], v_v = lim[1], w_hdg = lim[2], a_h = lim[3], a_v = lim[4], a_hdg = lim[5], j_h = lim[6], j_v = lim[7];
  const double* s = wp + (size_t)i * 4;
  const double* e = s + 4;
  Segment c;
  c.flags = 0;
  c.has_pre = i >= 1, c.has_post = i < S - 1;
  c.d[0] = e[0] - s[0], c.d[1] = e[1] - s[1], c.d[2] = e[2] - s[2];
  const double dx = c.d[0], dy = c.d[1], dz = c.d[2];
  const double distance = sqrt(dx * dx + dy * dy + dz * dz);
  c.D = distance;
  c.h = sqrt(dx * dx + dy * dy);
  const double inclinator = atan2(dz, sqrt(dx * dx + dy * dy));
  const Limit V = limit_for_inclination(inclinator, v_v, v_h, th.thr[0]);
  const Limit A = limit_for_inclination(inclinator, a_v, a_h, th.thr[1]);
  const Limit J = limit_for_inclination(inclinator, j_v, j_h, th.thr[2]);
  const double v_max = V.value, a_max = A.value, j_max = J.value;
  c.flags |= (V.vertical ? kVVertical : 0) | (A.vertical ? kAVertical : 0) | (J.vertical ? kJVertical : 0);
  double t1 = 0, t2 = 0;
  const double full = (v_max / a_max) + (a_max / j_max);
  unit3(s, e, c.u2);
  c.n1 = c.n3 = c.dot1 = c.dot2 = 0.0;
  for (int k = 0; k < 3; ++k) c.u1[k] = c.u3[k] = 0.0;
  if (i >= 1) {
    c.n1 = unit3(wp + (size_t)(i - 1) * 4, s, c.u1);
    const double dot = c.u1[0] * c.u2[0] + c.u1[1] * c.u2[1] + c.u1[2] * c.u2[2];
    c.dot1 = dot;
    if (dot < 0) c.flags |= kDot1Clamped;
    t1 = (1 - (dot < 0 ? 0.0 : dot)) * full;
  }
  if (i == 0) t1 = full;
  if (i == S - 1) t2 = full;
  if (i < S - 1) {
    c.n3 = unit3(e, wp + (size_t)(i + 2) * 4, c.u3);
    const double dot = c.u2[0] * c.u3[0] + c.u2[1] * c.u3[1] + c.u2[2] * c.u3[2];
    c.dot2 = dot;
    if (dot < 0) c.flags |= kDot2Clamped;
    t2 = (1 - (dot < 0 ? 0.0 : dot)) * full;
  }
  const double cap = sqrt(2 * distance / a_max);
  c.t1_raw = t1, c.t2_raw = t2, c.cap = cap;
  if (cap < t1) t1 = cap, c.flags |= kT1Capped;  // std::min(t1, cap): the reference's `t1 > cap`
  if (cap < t2) t2 = cap, c.flags |= kT2Capped;
  double t = distance / v_max + t1 + t2;
  c.t_dist = t;
  if (t < kFloorTime) t = kFloorTime, c.flags |= kFloor;
  c.delta = radians_diff(s[3], e[3]);
  const double ang = fabs(c.delta);
  c.ang = ang;
  double tv = 0, ta = 0;
  c.relaxed = !(w_hdg < (double)FLT_MAX && a_hdg < (double)FLT_MAX);
  c.ang_cruise = 0.0;
  if (!c.relaxed) {
    c.ang_cruise = 2 * (w_hdg * w_hdg) / a_hdg;
    const double reduced = (ang - 2 * (w_hdg * w_hdg) / a_hdg) / w_hdg;
    if (!(reduced < 0)) c.flags |= kHeadingCruise;
    tv = (reduced < 0) ? ang / w_hdg : reduced;
    if (ang > kPi / 4) {
      c.flags |= kHeadingAcc;
      ta = 2 * (w_hdg / a_hdg);
    }
  }
  const double hf = 1.5 * (tv + ta);
  c.hf = hf;
  if (hf > t) t = hf, c.flags |= kHeading;  // (a tie stays with the distance term)
  c.value = t;
  c.inclinator = inclinator, c.thr[0] = V.thr, c.thr[1] = A.thr, c.thr[2] = J.thr;
  bool usable = finite(t);
  for (int k = 0; k < 8; ++k) usable = usable && finite(s[k]) && lim[k] == lim[k];
  if (c.has_pre)
    for (int k = 0; k < 3; ++k) usable = usable && finite(s[k - 4]);
  if (c.has_post)
    for (int k = 0; k < 3; ++k) usable = usable && finite(e[4 + k]);
  if (!usable) c.flags = kFloor;
  return c;
}

// G dt/d(pre, s, e, post) and G dt/dlimits of one segment
struct Partials {
  double pre[3], start[4], end[4], post[3];
  double lim[kLimits];
};

// one of v, a, j in the gradient's form: L_max = c D / q
struct Regime {
  int index;            // the limit entry c is
  double c, q, gq[3];   // grad q with respect to the end waypoint
  double rho[3];        // grad q / q
  double value;         // c D / q
};
MRS_TG_HD inline Regime regime(const Segment& s, bool vertical, int group, const double* lim) {
  MRS_TG_NO_CONTRACT
  Regime r;
  r.index = 3 * group + (vertical ? 1 : 0);
  r.c = lim[r.index];
  if (vertical) {
    r.q = fabs(s.d[2]);
    r.gq[0] = r.gq[1] = 0.0, r.gq[2] = sign_of(s.d[2]);
  } else {
    r.q = s.h;
    r.gq[0] = s.d[0] / s.h, r.gq[1] = s.d[1] / s.h, r.gq[2] = 0.0;
  }
  for (int k = 0; k < 3; ++k) r.rho[k] = r.gq[k] / r.q;
  r.value = r.c * s.D / r.q;
  return r;
}

MRS_TG_HD inline Partials partials(const Segment& s, const double* lim, double G) {
  MRS_TG_NO_CONTRACT
  Partials p;
  for (int k = 0; k < 3; ++k) p.pre[k] = p.post[k] = 0.0;
  for (int k = 0; k < 4; ++k) p.start[k] = p.end[k] = 0.0;
  for (int k = 0; k < kLimits; ++k) p.lim[k] = 0.0;
  if (G == 0.0) return p;
  if (s.flags & kHeading) {
    const double w = lim[2], a = lim[5];
    const bool cruise = (s.flags & kHeadingCruise) != 0, acc = (s.flags & kHeadingAcc) != 0;
    p.end[3] = G * (0.0 - 1.5 * (sign_of(s.delta) / w));
    p.start[3] = 0.0 - p.end[3];
    double dw = 0.0 - s.ang / (w * w);
    if (cruise) dw = dw - 2.0 / a;
    if (acc) dw = dw + 2.0 / a;
    p.lim[2] = G * (1.5 * dw);
    const double q = 2.0 * (w / (a * a));
    double da = 0.0;
    if (cruise) da = da + q;
    if (acc) da = da - q;
    p.lim[5] = G * (1.5 * da);
    return p;
  }
  if (s.flags & kFloor) return p;
  const Regime V = regime(s, (s.flags & kVVertical) != 0, 0, lim), A = regime(s, (s.flags & kAVertical) != 0, 1, lim),
               J = regime(s, (s.flags & kJVertical) != 0, 2, lim);
  if (V.q == 0.0 || A.q == 0.0 || J.q == 0.0) return p;  // (a segment without length is FLOOR or HEADING)
  const double r_va = V.value / A.value, r_aj = A.value / J.value;
  const double full = r_va + r_aj;
  const double half_cap = 0.5 * sqrt(2 * s.D / A.value);
  double f1[3], f2[3], cp[3];  // dfull/de in its two addends, dcap/de
  for (int k = 0; k < 3; ++k) {
    f1[k] = r_va * (A.rho[k] - V.rho[k]);
    f2[k] = r_aj * (J.rho[k] - A.rho[k]);
    cp[k] = half_cap * A.rho[k];
  }
  const bool capped1 = (s.flags & kT1Capped) != 0, capped2 = (s.flags & kT2Capped) != 0;
  const bool smooth1 = s.has_pre && !capped1 && !(s.flags & kDot1Clamped);
  const bool smooth2 = s.has_post && !capped2 && !(s.flags & kDot2Clamped);
  const double c1 = smooth1 ? 1 - s.dot1 : 1.0, c2 = smooth2 ? 1 - s.dot2 : 1.0;
  const bool own = s.D * s.D > 0, front = s.n1 * s.n1 > 0, behind = s.n3 * s.n3 > 0;
  double se[3], ss[3], sp[3], sq[3];
  for (int k = 0; k < 3; ++k) {
    double end = 0.0, start = 0.0, pre = 0.0, post = 0.0;
    const double a0 = V.gq[k] / V.c;  // D / v_max
    end = accumulate(end, a0);
    start = accumulate(start, 0.0 - a0);
    if (capped1) {
      end = accumulate(end, cp[k]);
      start = accumulate(start, 0.0 - cp[k]);
    } else {
      end = accumulate(end, c1 * f1[k]);
      end = accumulate(end, c1 * f2[k]);
      start = accumulate(start, 0.0 - c1 * f1[k]);
      start = accumulate(start, 0.0 - c1 * f2[k]);
      if (smooth1 && own) {  // dot1 through d = e - s
        const double x1 = full * (s.u1[k] / s.D), x2 = full * ((s.dot1 * s.u2[k]) / s.D);
        end = accumulate(end, 0.0 - x1);
        end = accumulate(end, x2);
        start = accumulate(start, x1);
        start = accumulate(start, 0.0 - x2);
      }
      if (smooth1 && front) {  // dot1 through s - pre
        const double y1 = full * (s.u2[k] / s.n1), y2 = full * ((s.dot1 * s.u1[k]) / s.n1);
        start = accumulate(start, 0.0 - y1);
        start = accumulate(start, y2);
        pre = accumulate(pre, y1);
        pre = accumulate(pre, 0.0 - y2);
      }
    }
    if (capped2) {
      end = accumulate(end, cp[k]);
      start = accumulate(start, 0.0 - cp[k]);
    } else {
      end = accumulate(end, c2 * f1[k]);
      end = accumulate(end, c2 * f2[k]);
      start = accumulate(start, 0.0 - c2 * f1[k]);
      start = accumulate(start, 0.0 - c2 * f2[k]);
      if (smooth2 && own) {  // dot2 through d = e - s
        const double x1 = full * (s.u3[k] / s.D), x2 = full * ((s.dot2 * s.u2[k]) / s.D);
        end = accumulate(end, 0.0 - x1);
        end = accumulate(end, x2);
        start = accumulate(start, x1);
        start = accumulate(start, 0.0 - x2);
      }
      if (smooth2 && behind) {  // dot2 through post - e
        const double y1 = full * (s.u2[k] / s.n3), y2 = full * ((s.dot2 * s.u3[k]) / s.n3);
        end = accumulate(end, y1);
        end = accumulate(end, 0.0 - y2);
        post = accumulate(post, 0.0 - y1);
        post = accumulate(post, y2);
      }
    }
    se[k] = end, ss[k] = start, sp[k] = pre, sq[k] = post;
  }
  for (int k = 0; k < 3; ++k) {
    p.end[k] = G * se[k];
    p.start[k] = G * ss[k];
    p.pre[k] = G * sp[k];
    p.post[k] = G * sq[k];
  }
  // the limits: the entries of c_v, c_a and c_j (three different entries), each D / v_max first, then side 1, then side 2
  double sv = 0.0, sa = 0.0, sj = 0.0;
  sv = accumulate(sv, 0.0 - (V.q / V.c) / V.c);
  for (int side = 0; side < 2; ++side) {
    if (side == 0 ? capped1 : capped2) {
      sa = accumulate(sa, 0.0 - half_cap / A.c);
    } else {
      const double c = side == 0 ? c1 : c2;
      sv = accumulate(sv, c * (r_va / V.c));
      sa = accumulate(sa, 0.0 - c * (r_va / A.c));
      sa = accumulate(sa, c * (r_aj / A.c));
      sj = accumulate(sj, 0.0 - c * (r_aj / J.c));
    }
  }
  const double gv = G * sv, ga = G * sa, gj = G * sj;
  p.lim[0] = V.index == 0 ? gv : 0.0, p.lim[1] = V.index == 1 ? gv : 0.0;
  p.lim[3] = A.index == 3 ? ga : 0.0, p.lim[4] = A.index == 4 ? ga : 0.0;
  p.lim[6] = J.index == 6 ? gj : 0.0, p.lim[7] = J.index == 7 ? gj : 0.0;
  return p;
}

// dL/dwaypoint of vertex j (0 .. S) of a path: wp the path's first waypoint row, G its S upstream entries (null: the flags
// alone are wanted).  flags_out: the flags of the segment that starts at j (j < S), may be null.
// (Role is a compile-time constant so that each of the four visits keeps only the part of partials() it reads)
template <int Role>
MRS_TG_HD inline void vertex_part(const double* wp, const double* G, int j, int S, const double* lim, const Thresholds& th,
                                  double (&g)[4], int* flags_out) {
  const int seg = j - 2 + Role;
  if (seg < 0 || seg >= S) return;
  const bool report = Role == 2 && flags_out;
  if (!G && !report) return;
  const Segment c = classify(wp, seg, S, lim, th);
  if (report) *flags_out = c.flags;
  if (!G) return;
  const Partials p = partials(c, lim, G[seg]);
  const double* part = Role == 0 ? p.post : Role == 1 ? p.end : Role == 2 ? p.start : p.pre;
  for (int k = 0; k < (Role == 1 || Role == 2 ? 4 : 3); ++k) g[k] = accumulate(g[k], part[k]);
}
MRS_TG_HD inline void vertex_gradient(const double* wp, const double* G, int j, int S, const double* lim, double (&g)[4],
                                      int* flags_out) {
  for (int k = 0; k < 4; ++k) g[k] = 0.0;
  const Thresholds th = thresholds(lim);
  vertex_part<0>(wp, G, j, S, lim, th, g, flags_out);  // post of j - 2, end of j - 1, start of j, pre of j + 1:
  vertex_part<1>(wp, G, j, S, lim, th, g, flags_out);  // increasing segment index
  vertex_part<2>(wp, G, j, S, lim, th, g, flags_out);
  vertex_part<3>(wp, G, j, S, lim, th, g, flags_out);
}

// dL/dlimits of one path: its segments in increasing index; entry 8 stays 0
MRS_TG_HD inline void limit_gradient(const double* wp, const double* G, int S, const double* lim, double (&g)[kLimits]) {
  for (int k = 0; k < kLimits; ++k) g[k] = 0.0;
  const Thresholds th = thresholds(lim);
  for (int j = 0; j < S; ++j) {
    const Partials p = partials(classify(wp, j, S, lim, th), lim, G[j]);
    for (int k = 0; k < kLimits - 1; ++k) g[k] = accumulate(g[k], p.lim[k]);
  }
}

// the nodelet's gate on the optimiser's code (mrs_trajectory_generation.cpp:1138-1149): >= 1 except 6 (MAXTIME), and -1
MRS_TG_HD inline bool code_accepted(int status) { return (status >= 1 && status != 6) || status == -1; }

// the length sanity check (:1178-1199): 0 = passes, +1 = "too long", -1 = "too short" (or the two codes the caller names: the
// plan step's verdicts).  Only trajectories longer than one second are checked; a factor <= 0 switches its side of the check
// off (the reference has no such switch: its parameters are always loaded, config/public/trajectory_generation.yaml:35-36)
MRS_TG_HD inline int length_check(int n_samples, double dt, double total, double max_factor, double min_factor, int too_long = 1,
                                  int too_short = -1) {
  MRS_TG_NO_CONTRACT
  const double len = (double)n_samples * dt;
  if (!(len > 1.0)) return 0;
  if (max_factor > 0 && len > max_factor * total) return too_long;
  if (min_factor > 0 && len < min_factor * total) return too_short;
  return 0;
}

// initial_total_time_baca, code_accepted and length_check for one path: the total from 0.0 in increasing index; status
// null = no code to reject on
struct Gate {
  double total;
  int verdict;
};
MRS_TG_HD inline Gate length_gate(const double* seg_times, int S, int n_samples, double dt, double max_factor, double min_factor,
                                  const int32_t* status) {
  MRS_TG_NO_CONTRACT
  Gate g;
  double tot = 0;
  for (int j = 0; j < S; ++j) tot += seg_times[j];
  g.total = tot;
  g.verdict = kVerdictAccepted;
  if (status && !code_accepted(*status)) {
    g.verdict = kVerdictCode;
    return g;
  }
  static_assert(kVerdictAccepted == 0, "length_check's `passes`");
  g.verdict = length_check(n_samples, dt, tot, max_factor, min_factor, kVerdictTooLong, kVerdictTooShort);
  return g;
}

}  // namespace baca
}  // namespace mrs_tg

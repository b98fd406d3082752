// mrs_tg_request.hpp -- the two pieces of findTrajectory() that turn a request into the solver's inputs, as the plan steps run
// them (mrs_tg_request.hip: mrs_tg_plan_request_vertices, mrs_tg_plan_request_limits and their backward passes); DESIGN.md
// section 11h.  The stages are the vertices (mrs_trajectory_generation.cpp:923-977 of the reference) and the limits (:981-1038;
// findTrajectoryFallback's variant :1252-1299).  This is the one definition of the vertex rule and of the limits' two tail steps
// under csrc/: the policy layer (mrs_tg_policy_host.hpp, policy_expand_kernel) calls it.  limits_for (include/mrs_tg_service.hpp)
// is the public header's own statement; tests/host/request_harness.cpp holds this file to restatements of the reference's lines.
//   vertices     the headings unwrapped along the path, THE CHAIN h_i = unwrap(raw_i, h_{i-1}) STARTING FROM THE STATE'S HEADING
//                where the path has a state and from the first raw heading where it has none (fbq::unwrap, the one copy); every
//                vertex constrains its position, the ends their derivatives 1 .. d, the first vertex of a path with a state its
//                derivatives 1 .. 3 to the state's rows, a stop_at vertex between the ends its derivatives 1 .. 3 to zero.
//   limits       lim[9] = {v_h, v_v, v_hdg, a_h, a_v, a_hdg, j_h, j_v, j_hdg} from the constraints c[12], the override o[6]
//                with its can_change test against the state, the relaxed heading and the fallback's two factors, with the
//                branch word (MRS_TG_LIM_*) the backward pass is driven by.
// Every value is a copy of an input, except the unwrapped heading (the input plus a piecewise-constant multiple of 2 pi) and the
// four limits the fallback scales (one multiplication).  The comparisons are the C++ comparisons as written: a NaN in an
// operand of can_change refuses the override, (desc < asc) ? desc : asc is std::min(asc, desc).  Plain double,
// __host__ __device__, no contraction; the library functions are fmod (inside unwrap), hypot and fabs.
#pragma once

#include <cfloat>

#include "mrs_tg_baca.hpp"
#include "mrs_tg_fallback.hpp"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace reqq {

using mrs_tg::accumulate;

constexpr int kConstraints = 12, kOverrides = 6, kLimits = 9, kState = 16, kVertexValues = kB * kD;
constexpr int kChunk = 64;  // vertices a wavefront takes at a time: one per lane

// flags_dev of mrs_tg_plan_request_limits (MRS_TG_REQ_*) and its branch word (MRS_TG_LIM_*): the values of include/mrs_tg.h
// (mrs_tg_request.hip asserts that they are the same)
constexpr int32_t kReqOverride = 1, kReqRelaxHeading = 2;
constexpr int32_t kOverridden = 1, kOverrideRefused = 2, kRelaxed = 4, kVDescending = 8, kADescending = 16, kJDescending = 32,
                  kFallback = 64;

// ---- the vertices ---------------------------------------------------------------------------------------------------------------

// what the chain starts from (:925): the state's heading, state[0][3], or the first raw heading
MRS_TG_HD inline double chain_start(bool has_state, const double* state, const double* raw) { return has_state ? state[3] : raw[3]; }

// the mask [5] of a vertex (:940-976): first / last of its path, has_state and stop as the caller knows them
MRS_TG_HD inline void vertex_mask(bool first, bool last, bool has_state, bool stop, int d, uint8_t (&m)[kB]) {
  m[0] = 1;
  MRS_TG_UNROLL
  for (int k = 1; k < kB; ++k) m[k] = 0;
  if (first || last) {
    MRS_TG_UNROLL
    for (int k = 1; k < kB; ++k)
      if (k <= d) m[k] = 1;
    if (first && has_state) m[1] = m[2] = m[3] = 1;  // (d = 2 too: the state's rows 1 .. 3 are always pinned)
  } else if (stop) {
    m[1] = m[2] = m[3] = 1;
  }
}

// the values [5][4] of a vertex: its unwrapped waypoint, the state's rows 1 .. 3 at the first vertex of a path that has one,
// +0.0 everywhere else
MRS_TG_HD inline void vertex_values(const double (&w)[kD], bool first_with_state, const double* state, double (&val)[kVertexValues]) {
  MRS_TG_UNROLL
  for (int e = 0; e < kVertexValues; ++e) val[e] = 0.0;
  MRS_TG_UNROLL
  for (int k = 0; k < kD; ++k) val[k] = w[k];
  if (first_with_state) {
    MRS_TG_UNROLL
    for (int e = kD; e < 4 * kD; ++e) val[e] = state[e];
  }
}

// one path, serially: raw [V][4], stop_at [V] or null, state [4][4] (read where has_state); every output may be null, wp_out may
// be raw
MRS_TG_HD inline void vertices(const double* raw, const uint8_t* stop_at, int V, bool has_state, const double* state, int d,
                               double* wp_out, uint8_t* mask_out, double* vals_out) {
  double last = V > 0 ? chain_start(has_state, state, raw) : 0.0;
  for (int i = 0; i < V; ++i) {
    double w[kD];
    for (int k = 0; k < 3; ++k) w[k] = raw[(size_t)i * 4 + k];
    w[3] = fbq::unwrap(raw[(size_t)i * 4 + 3], last);
    last = w[3];
    if (wp_out)
      for (int k = 0; k < kD; ++k) wp_out[(size_t)i * 4 + k] = w[k];
    if (mask_out) {
      uint8_t m[kB];
      vertex_mask(i == 0, i == V - 1, has_state, stop_at != nullptr && stop_at[i] != 0, d, m);
      for (int k = 0; k < kB; ++k) mask_out[(size_t)i * kB + k] = m[k];
    }
    if (vals_out) {
      double val[kVertexValues];
      vertex_values(w, i == 0 && has_state, state, val);
      for (int e = 0; e < kVertexValues; ++e) vals_out[(size_t)i * kVertexValues + e] = val[e];
    }
  }
}

// backward, one vertex: dL/draw[i][:] = g_wp[i][:] + g_vals[i][0][:], one addition, a null upstream counting as zero
// (dh_i/draw_i = 1: the unwrap adds a piecewise-constant multiple of 2 pi); g_wp, g_vals: the vertex's own row and block or null
MRS_TG_HD inline void vertex_vjp(const double* g_wp, const double* g_vals, double (&g_raw)[kD]) {
  MRS_TG_UNROLL
  for (int k = 0; k < kD; ++k) g_raw[k] = accumulate(g_wp ? g_wp[k] : 0.0, g_vals ? g_vals[k] : 0.0);
}
// ... and one path's state block [4][4]: rows 1 .. 3 the upstream on the first vertex's value rows 1 .. 3 where the path has a
// state, zeros otherwise; row 0 zeros (dh_i/d(state heading) = 0)
MRS_TG_HD inline void state_vjp(bool has_state, const double* g_vals_first, double (&g_state)[kState]) {
  MRS_TG_UNROLL
  for (int e = 0; e < kState; ++e) g_state[e] = (has_state && g_vals_first && e >= kD) ? g_vals_first[e] : 0.0;
}

// ---- the limits -----------------------------------------------------------------------------------------------------------------

// where lim[k] comes from: the constraint entry (the ascending one of a vertical pair, the descending one right behind it) and
// the override entry (-1: the heading limits have none)
struct LimitSource {
  int c, o;
  bool vertical;
};
MRS_TG_HD constexpr LimitSource limit_source(int k) {
  // k:            v_h          v_v          v_hdg          a_h          a_v          a_hdg          j_h          j_v          j_hdg
  return k == 0   ? LimitSource{0, 0, false}
         : k == 1 ? LimitSource{3, 1, true}
         : k == 2 ? LimitSource{9, -1, false}
         : k == 3 ? LimitSource{1, 2, false}
         : k == 4 ? LimitSource{5, 3, true}
         : k == 5 ? LimitSource{10, -1, false}
         : k == 6 ? LimitSource{2, 4, false}
         : k == 7 ? LimitSource{7, 5, true}
                  : LimitSource{11, -1, false};
}
// the bit of the branch word that says a vertical pair's descending value was taken
MRS_TG_HD constexpr int32_t descending_bit(int k) { return k == 1 ? kVDescending : (k == 4 ? kADescending : kJDescending); }
// the fallback's factor on lim[k] (:1295-1299): the speed factor on 0 and 1, the acceleration factor on 3 and 4
MRS_TG_HD inline bool fallback_scaled(int k) { return k == 0 || k == 1 || k == 3 || k == 4; }
MRS_TG_HD inline double fallback_factor(int k, double speed_factor, double accel_factor) { return k < 3 ? speed_factor : accel_factor; }
// the two tail steps of the limits, on a lim[9] row: relax_heading (:1030-1038) and the fallback's two factors (:1295-1299)
MRS_TG_HD inline void relax_heading_limits(double* lim) { lim[2] = lim[5] = lim[8] = (double)FLT_MAX; }
MRS_TG_HD inline void scale_fallback_limits(double* lim, double speed_factor, double accel_factor) {
  MRS_TG_NO_CONTRACT
  MRS_TG_UNROLL
  for (int k = 0; k < kLimits; ++k)
    if (fallback_scaled(k)) lim[k] = lim[k] * fallback_factor(k, speed_factor, accel_factor);
}

// can_change of :1001-1008: six strict comparisons of the state (rows 1 .. 3 = velocity, acceleration, jerk) with the override
MRS_TG_HD inline bool can_change(const double* state, const double* o) {
  return hypot(state[4], state[5]) < o[0] && hypot(state[8], state[9]) < o[2] && hypot(state[12], state[13]) < o[4] &&
         fabs(state[6]) < o[1] && fabs(state[10]) < o[3] && fabs(state[14]) < o[5];
}

// one path: c [12], o [6] (read where flags has kReqOverride), state [4][4] (read where has_state) -> lim [9], the branch word
MRS_TG_HD inline int32_t limits(const double* c, const double* o, int32_t flags, bool has_state, const double* state, bool fallback,
                                double speed_factor, double accel_factor, double (&lim)[kLimits]) {
  MRS_TG_NO_CONTRACT
  int32_t branch = fallback ? kFallback : 0;
  MRS_TG_UNROLL
  for (int k = 0; k < kLimits; ++k) {
    const LimitSource s = limit_source(k);
    double v = c[s.c];
    if (s.vertical) {
      const double asc = c[s.c], desc = c[s.c + 1];
      if (desc < asc) v = desc, branch |= descending_bit(k);  // std::min(asc, desc): a tie takes the ascending value
    }
    lim[k] = v;
  }
  if (flags & kReqOverride) {
    // findTrajectory tests the override against the state (:997-1026); findTrajectoryFallback takes it as it is (:1259-1267)
    const bool take = fallback || !has_state || can_change(state, o);
    if (take) {
      MRS_TG_UNROLL
      for (int k = 0; k < kLimits; ++k)
        if (limit_source(k).o >= 0) lim[k] = o[limit_source(k).o];
    }
    branch |= take ? kOverridden : kOverrideRefused;
  }
  if (flags & kReqRelaxHeading) {
    relax_heading_limits(lim);
    branch |= kRelaxed;
  }
  if (fallback) scale_fallback_limits(lim, speed_factor, accel_factor);  // after the override, as the reference does
  return branch;
}

// backward, one path, the branch word held fixed: g_lim [9] -> g_c [12], g_o [6], every element written.  The entry that
// supplied a value gets its gradient (times the fallback's factor on 0, 1, 3, 4): the override entry where overridden, else the
// winning side of the min; a relaxed heading limit gives nothing; the state gets nothing.
MRS_TG_HD inline void limits_vjp(int32_t branch, bool fallback, double speed_factor, double accel_factor, const double* g_lim,
                                 double (&g_c)[kConstraints], double (&g_o)[kOverrides]) {
  MRS_TG_NO_CONTRACT
  MRS_TG_UNROLL
  for (int e = 0; e < kConstraints; ++e) g_c[e] = 0.0;
  MRS_TG_UNROLL
  for (int e = 0; e < kOverrides; ++e) g_o[e] = 0.0;
  MRS_TG_UNROLL
  for (int k = 0; k < kLimits; ++k) {
    const LimitSource s = limit_source(k);
    double g = g_lim[k];
    if (fallback && fallback_scaled(k)) g = g * fallback_factor(k, speed_factor, accel_factor);
    if (s.o >= 0) {
      if (branch & kOverridden) {
        g_o[s.o] = g;
      } else if (s.vertical) {
        const bool desc = (branch & descending_bit(k)) != 0;
        g_c[s.c] = desc ? 0.0 : g;
        g_c[s.c + 1] = desc ? g : 0.0;
      } else {
        g_c[s.c] = g;
      }
    } else if (!(branch & kRelaxed)) {
      g_c[s.c] = g;
    }
  }
}

}  // namespace reqq
}  // namespace mrs_tg

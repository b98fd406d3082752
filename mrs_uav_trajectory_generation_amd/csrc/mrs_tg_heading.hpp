// mrs_tg_heading.hpp -- the heading along the direction of travel (mrs_tg_plan_travel_heading, travel_heading_kernel) and its
// backward pass (mrs_tg_plan_travel_heading_vjp, travel_heading_vjp_kernel); DESIGN.md section 11f.  The stage is
// getTrajectoryReference with override_heading_atan2 (mrs_trajectory_generation.cpp:1578-1603 of the reference): for the rows
// i = 0 .. n-2 of a path of n samples
//   (dx, dy) = (x, y)_{i+1} - (x, y)_i,   dist = sqrt(dx dx + dy dy)
//   heading_i = heading_{i-1}        if dist < min_step and i > 0        (a row that barely moves keeps the heading in front)
//             = atan2(dy, dx)        otherwise                           (row i is a SOURCE)
// and row n-1 keeps its own.  "Keeps" chains: a run of slow rows carries the value of the last source in front of it, so
// heading_i = atan2 of the step of source(i), the highest source at or below i -- a copy of those bits, not a second atan2.
// The reference decides on std::hypot(dy, dx); dist is written out, so that the harness under g++ and the kernel execute the
// same operations.  The two distances are within an ulp of each other: the decision can differ from the host loop's
// (mrs_tg_policy_host.hpp) only for a step within an ulp of min_step.  atan2 is the one place a libm enters: the device's in
// the kernel, the host's in the harness.  No product is contracted into a fused multiply-add.  Plain double,
// __host__ __device__: tests/host/heading_harness.cpp runs this file under g++.  The host loop takes kMinStep, is_source and
// heading_of from here and keeps std::hypot for its distance: the rule and its constant are written in this file only.
//
// Backward, sources held fixed.  A source s with the rows s .. e-1 of its run (e the next source, at most n-1) collects
//   G_s = dL/dheading_s + ... + dL/dheading_{e-1}      from 0.0, in increasing row index (accumulate)
// and atan2_rows gives, with r2 = dx dx + dy dy of its step, row s (+dy/r2 G, -dx/r2 G) and row s+1 (-dy/r2 G, +dx/r2 G), both
// exactly 0 when r2 == 0.  THE ORDER OF THE TERMS of a row's x (and y): the passed-through upstream, then the term of the row's
// own step, then the term of the step of the row in front; a term that does not exist is not added.
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace hdg {

using mrs_tg::accumulate;

constexpr double kMinStep = 0.05;  // :1590, a constant of the reference

// the step from row a to row b in the plane (x, y are read)
struct Step {
  double dx, dy, dist;
};
MRS_TG_HD inline Step step_xy(const double* a, const double* b) {
  MRS_TG_NO_CONTRACT
  Step s;
  s.dx = b[0] - a[0];
  s.dy = b[1] - a[1];
  s.dist = sqrt(s.dx * s.dx + s.dy * s.dy);
  return s;
}

// whether row i takes the direction of its own step: the reference's condition (:1590), negated.  Row 0 always does (on a zero
// step atan2(0, 0) = 0); a distance that is not a number does, and gives a heading that is not a number, as on the host.
MRS_TG_HD inline bool is_source(int i, double dist, double min_step) { return !(dist < min_step && i > 0); }

MRS_TG_HD inline double heading_of(double dx, double dy) { return atan2(dy, dx); }

// g * d atan2(dy, dx) / d(row a), d(row b): ra the step's first sample (x, y), rb the next one
MRS_TG_HD inline void atan2_rows(double dx, double dy, double g, double (&ra)[2], double (&rb)[2]) {
  MRS_TG_NO_CONTRACT
  ra[0] = ra[1] = rb[0] = rb[1] = 0.0;
  const double r2 = dx * dx + dy * dy;
  if (r2 == 0.0) return;
  const double tx = dy / r2 * g, ty = dx / r2 * g;
  ra[0] = tx, ra[1] = 0.0 - ty;
  rb[0] = 0.0 - tx, rb[1] = ty;
}

}  // namespace hdg
}  // namespace mrs_tg

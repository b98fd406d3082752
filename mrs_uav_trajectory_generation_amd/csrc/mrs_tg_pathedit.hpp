// mrs_tg_pathedit.hpp -- the two stages of optimize() that change the number of waypoints of a path, as plan steps, and their one
// backward pass (mrs_tg_plan_preprocess_path, mrs_tg_plan_insert_midpoints, mrs_tg_plan_path_edit_vjp; thin_path_kernel,
// insert_midpoints_kernel, path_edit_vjp_kernel).  Thinning is preprocessPath
// (src/mrs_trajectory_generation.cpp:431-500 of the reference), subdivision the mid-point insertion behind
// validateTrajectorySpatial (:739-753).  Plain double, __host__ __device__ (section 4a): policy::preprocess and
// policy::insert_midpoints (mrs_tg_policy_host.hpp) call this file, tests/host/pathedit_harness.cpp runs it under g++, the
// kernels run it on the device.  No product is contracted into a fused multiply-add and no libm function beyond sqrt and fmod
// is called: the host's bits on the device.
//
// THINNING, one candidate.  keeps(wp, n, last, i, o) says whether input vertex i of a path of n vertices is kept, given that
// input vertex `last` was the last one kept -- what one iteration of the reference's loop decides:
//   i == 0 and i == n - 1 are kept;
//   0 < i < n - 1, the straightener first (enabled, n >= 3): every j in (last, i] against the segment wp[last] -> wp[i + 1]; the
//     vertex is dropped when none of them has dist > max_deviation nor either SIGNED heading comparison of quirk B3;
//   else it is dropped when sqrt(dx^2 + dy^2 + dz^2) < min_waypoint_distance against wp[last].
// Comparisons are written as the host writes them: a NaN compares false everywhere, so a NaN coordinate is kept by the distance
// test and passes the straightener's.  The scan is serial in the KEPT vertices only: between two kept vertices every candidate
// is judged against the same `last`, so 64 candidates can be judged at once and the first kept one taken (thin_path below, with
// the window a wavefront uses).
//
// SUBDIVISION, one segment.  inserts(unsafe, s, first_segment, V): a mid-point goes into original segment s of a path of V
// vertices when the segment is unsafe AND (s > 0 OR first_segment OR V <= 2); V is the count before any insertion (the reference
// tests the size at its first iterator position only, where nothing has been inserted yet).  unsafe(segment_max, max_deviation)
// is segment_max > max_deviation: a NaN is never unsafe.  The mid-point is interpolate_point(a, b, 0.5).
//
// BACKWARD of both (edit_gradient).  The edited path is described by source[] (the input vertex an output vertex copies; for a
// mid-point the first vertex of its segment) and inserted[] (1 for a mid-point; absent after thinning); source is non-decreasing
// along a path.  Input vertex v's row starts at 0.0 and takes, in this order, 0.5 * g of the mid-point of the segment in front of
// it, g of its own copy, 0.5 * g of the mid-point of its own segment, each addend rounded and then added with accumulate().  All
// four columns alike: the heading column is the almost-everywhere derivative of radians::interp, its wrap held fixed.  A vertex
// without a copy (dropped by the thinning) gets a zero row.
#pragma once

#include "mrs_tg_baca.hpp"
#include "mrs_tg_deviation.hpp"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace pathq {

using baca::kPi;
using baca::radians_diff;
using baca::wrap_range;
using mrs_tg::accumulate;

constexpr int kWindow = 64;  // candidates judged at once: a wavefront

// mrs_lib radians::interp (angles into [0, 2 pi)): fmod, additions and comparisons
MRS_TG_HD inline double interp_heading(double from, double to, double c) {
  MRS_TG_NO_CONTRACT
  return wrap_range(from + c * radians_diff(to, from), 0.0, 2.0 * kPi);
}

// interpolatePoint (:1612-1625): a + coeff (b - a) for x, y, z, radians::interp for the heading
MRS_TG_HD inline void interpolate_point(const double* a, const double* b, double coeff, double* out) {
  MRS_TG_NO_CONTRACT
  MRS_TG_UNROLL
  for (int k = 0; k < 3; ++k) out[k] = a[k] + coeff * (b[k] - a[k]);
  out[3] = interp_heading(a[3], b[3], coeff);
}

struct ThinOptions {
  double min_waypoint_distance;
  int straightener_enabled;
  double straightener_max_deviation, straightener_max_hdg_deviation;
};

// whether input vertex i is kept behind the kept vertex `last`; wp: the path's n vertices, `stride` doubles apart (x, y, z, heading
// in front: 4 for the plan's rows, 5 for mrs_tg_waypoint)
MRS_TG_HD inline bool keeps(const double* wp, size_t stride, int n, int last, int i, const ThinOptions& o) {
  MRS_TG_NO_CONTRACT
  if (i <= 0 || i >= n - 1) return true;
  const double* first = wp + (size_t)last * stride;
  if (o.straightener_enabled && n >= 3) {
    const double* end = wp + (size_t)(i + 1) * stride;
    bool segment_is_ok = true;
    for (int j = last + 1; j < i + 1; ++j) {
      const double* mid = wp + (size_t)j * stride;
      // quirk B3 of the reference: fabs() wraps the comparison, so the heading test is signed
      if (devq::dist(mid, first, end) > o.straightener_max_deviation ||
          (radians_diff(first[3], mid[3]) > o.straightener_max_hdg_deviation) ||
          (radians_diff(end[3], mid[3]) > o.straightener_max_hdg_deviation)) {
        segment_is_ok = false;
        break;
      }
    }
    if (segment_is_ok) return false;
  }
  const double* w = wp + (size_t)i * stride;
  const double dx = first[0] - w[0], dy = first[1] - w[1], dz = first[2] - w[2];
  if (sqrt(dx * dx + dy * dy + dz * dz) < o.min_waypoint_distance) return false;
  return true;
}

MRS_TG_HD inline bool unsafe(double segment_max, double max_deviation) { return segment_max > max_deviation; }
MRS_TG_HD inline bool inserts(bool is_unsafe, int s, int first_segment, int V) {
  return is_unsafe && (s > 0 || first_segment != 0 || V <= 2);
}

// dL/d(input vertex v) [4] from the edited run of v's path: source / inserted / grad [n_run] (grad [n_run][4]; inserted may be
// null), v in the numbering source uses
MRS_TG_HD inline void edit_gradient(const int32_t* source, const uint8_t* inserted, int n_run, int v, const double* grad,
                                    double* g) {
  MRS_TG_NO_CONTRACT
  int lo = 0, hi = n_run;  // the first entry whose source is not below v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (source[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const bool copied = lo < n_run && source[lo] == v && !(inserted != nullptr && inserted[lo] != 0);
  if (copied) {
    if (inserted != nullptr && lo > 0 && inserted[lo - 1] != 0)
      for (int k = 0; k < 4; ++k) acc[k] = accumulate(acc[k], 0.5 * grad[(size_t)(lo - 1) * 4 + k]);
    for (int k = 0; k < 4; ++k) acc[k] = accumulate(acc[k], grad[(size_t)lo * 4 + k]);
    if (inserted != nullptr && lo + 1 < n_run && inserted[lo + 1] != 0 && source[lo + 1] == v)
      for (int k = 0; k < 4; ++k) acc[k] = accumulate(acc[k], 0.5 * grad[(size_t)(lo + 1) * 4 + k]);
  }
  for (int k = 0; k < 4; ++k) g[k] = acc[k];
}

// ---- the harness's and the policy layer's serial loops -----------------------------------------------------------------
// thin_path_serial is the reference's loop as policy::preprocess runs it; thin_path judges kWindow candidates against one `last`
// and takes the first kept one, as thin_path_kernel does with a ballot -- the same rows (tests/test_pathedit_host.py).

// kept [<= n]: the input index of every kept vertex -> their number
MRS_TG_HD inline int thin_path_serial(const double* wp, size_t stride, int n, const ThinOptions& o, int32_t* kept) {
  int count = 0, last = 0;
  for (int i = 0; i < n; ++i) {
    if (!keeps(wp, stride, n, last, i, o)) continue;
    kept[count++] = i;
    last = i;
  }
  return count;
}

MRS_TG_HD inline int thin_path(const double* wp, size_t stride, int n, const ThinOptions& o, int32_t* kept) {
  if (n <= 0) return 0;
  int count = 1, last = 0, base = 1;
  kept[0] = 0;
  while (base < n) {
    int first_kept = -1;
    for (int lane = 0; lane < kWindow && first_kept < 0; ++lane)
      if (base + lane < n && keeps(wp, stride, n, last, base + lane, o)) first_kept = lane;
    if (first_kept < 0) {
      base += kWindow;
      continue;
    }
    last = base + first_kept;
    kept[count++] = last;
    base = last + 1;
  }
  return count;
}

// the subdivided path of wp [V][4], stop_at [V] (may be null) under the flags unsafe_segment [V - 1]: out [<= 2 V - 1][4],
// stop_out, source_out (local input index), inserted_out (each may be null) -> the number of vertices
MRS_TG_HD inline int subdivide_path(const double* wp, const uint8_t* stop_at, int V, const uint8_t* unsafe_segment,
                                    int first_segment, double* out, uint8_t* stop_out, int32_t* source_out, uint8_t* inserted_out) {
  int n = 0;
  for (int i = 0; i < V; ++i) {
    for (int k = 0; k < 4; ++k) out[(size_t)n * 4 + k] = wp[(size_t)i * 4 + k];
    if (stop_out) stop_out[n] = stop_at ? stop_at[i] : 0;
    if (source_out) source_out[n] = i;
    if (inserted_out) inserted_out[n] = 0;
    ++n;
    if (i < V - 1 && inserts(unsafe_segment[i] != 0, i, first_segment, V)) {
      interpolate_point(wp + (size_t)i * 4, wp + (size_t)(i + 1) * 4, 0.5, out + (size_t)n * 4);
      if (stop_out) stop_out[n] = 0;
      if (source_out) source_out[n] = i;
      if (inserted_out) inserted_out[n] = 1;
      ++n;
    }
  }
  return n;
}

}  // namespace pathq
}  // namespace mrs_tg

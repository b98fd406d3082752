// mrs_tg_fallback.hpp -- the fallback sampler as a plan step, its backward pass and the heading unwrap
// (mrs_tg_plan_fallback_sample, mrs_tg_plan_fallback_sample_vjp, mrs_tg_plan_unwrap_headings; fallback_sample_kernel,
// fallback_sample_vjp_kernel, unwrap_headings_kernel).  The forward is the interpolation loop of
// findTrajectoryFallback (src/mrs_trajectory_generation.cpp:1327-1381 of the reference): constant-rate interpolation of the
// waypoint polyline on given segment times (the Baca estimate's), a dwell of `insert` repeated rows at a stop_at waypoint.
// Plain double, __host__ __device__ (section 4a): tests/host/fallback_harness.cpp runs this file under g++, the kernels run
// it on the device.
//
// THE ROW RULE.  Segment i of a path of S segments, its time t, the sampling step dt, insert = (int)round(stopping_time / dt)
// (computed once on the host):
//   nd      = (t > 0.1) ? ceil(t / dt) : 0.0          strictly; NaN and negative times give 0
//   emitted = nd + (nd > 0 && i == S - 1)             the last segment reaches the last waypoint
//   dwell   = (nd > 0 && i > 0 && stop_at[i]) ? insert : 0
//   rows    = emitted + dwell
//   step    = 1.0 / nd                                in double, never from a clamped integer
// Row r of the segment (0-based inside it): j = max(r - dwell, 0), coeff = (double)j * step,
//   p[k] = a[k] + coeff * (b[k] - a[k])   k = 0 .. 2, no fused multiply-add
//   p[3] = wrap_yaw(interp_heading(a[3], b[3], coeff))   on the raw headings, as :1362 does
// Counts are 64-bit integers; nd enters them clamped to 2^31 IN DOUBLE (a time of +inf takes part with that count), so nothing
// that does not fit is ever converted.  unwrap and interp_heading are fmod, additions and comparisons: the host's bits on the
// device.  wrap_yaw is the one place where the device's libm enters (sin, cos, atan2).
//
// BACKWARD, the counts held fixed (seg_times gets no gradient).  Row r of segment i with upstream row g [4] gives vertex i
// (1.0 - coeff) * g and vertex i + 1 coeff * g, all four columns alike: the heading column is the almost-everywhere derivative
// of wrap_yaw o interp_heading, its seams and the direction chosen at a heading difference of exactly +-pi held fixed.  THE
// ORDER OF THE SUMS: vertex v's row starts at 0.0, takes the rows of segment v - 1 in increasing row index, each addend
// coeff * g rounded and then added with accumulate(), then the rows of segment v in increasing row index, each addend
// (1.0 - coeff) * g.  Only rows below min(count, capacity) are read.
#pragma once

#include "mrs_tg_baca.hpp"
#include "mrs_tg_hd.hpp"
#include "mrs_tg_pathedit.hpp"

namespace mrs_tg {
namespace fbq {

using baca::kPi;
using baca::radians_diff;
using baca::wrap_range;
using mrs_tg::accumulate;
using pathq::interp_heading;  // mrs_lib radians::interp (angles into [0, 2 pi)): the one copy, mrs_tg_pathedit.hpp

constexpr double kMinSegmentTime = 1e-1;        // :1336, strictly
constexpr int32_t kMaxCapacity = 2147483646;   // the largest sample_capacity: capacity + 1, which the outputs report, fits int32
constexpr double kCountClamp = 2147483648.0;    // 2^31: what a segment's nd enters the 64-bit counts with at most

// mrs_lib sradians::unwrap: `what` brought to within pi of `from`.  The one definition: the policy layer and reqq call it
MRS_TG_HD inline double unwrap(double what, double from) {
  MRS_TG_NO_CONTRACT
  const double two_pi = 2.0 * kPi;
  double d = wrap_range(what, -kPi, two_pi) - wrap_range(from, -kPi, two_pi);
  if (d < -kPi) d += two_pi;
  else if (d >= kPi) d -= two_pi;
  return from + d;
}

// the yaw a sample carries after EigenTrajectoryPoint::setFromYaw / getYaw: quaternionFromYaw = (cos(y / 2), 0, 0, sin(y / 2)),
// yawFromQuaternion = atan2(2 (w z + x y), 1 - 2 (y^2 + z^2)) -- the round trip's own arithmetic
MRS_TG_HD inline double wrap_yaw(double y) {
  MRS_TG_NO_CONTRACT
  const double w = cos(y * 0.5), z = sin(y * 0.5);
  return atan2(2.0 * (w * z), 1.0 - 2.0 * (z * z));
}

// the headings of a path unwrapped in sequence (:1233-1241): vertex v against the unwrapped vertex v - 1, vertex 0 against
// itself; x, y, z copied.  out == in is allowed
MRS_TG_HD inline void unwrap_path(const double* wp, int n_vertices, double* out) {
  double last = n_vertices > 0 ? wp[3] : 0.0;
  for (int v = 0; v < n_vertices; ++v) {
    const double h = unwrap(wp[(size_t)v * 4 + 3], last);
    for (int k = 0; k < 3; ++k) out[(size_t)v * 4 + k] = wp[(size_t)v * 4 + k];
    out[(size_t)v * 4 + 3] = h;
    last = h;
  }
}

// (int)round(stopping_time / dt) as the host computes it once; false where it does not fit int32 (or is not a number)
MRS_TG_HD inline bool insert_count(double stopping_time, double dt, int32_t* insert) {
  MRS_TG_NO_CONTRACT
  const double r = round(stopping_time / dt);
  if (!(r >= 0.0 && r <= 2147483647.0)) return false;
  *insert = (int32_t)r;
  return true;
}

struct SegmentRows {
  double nd;       // ceil(t / dt), or 0: the divisor of the step
  int32_t dwell;   // rows inserted behind the segment's first
  long long rows;  // emitted + dwell, nd clamped to 2^31
};

MRS_TG_HD inline SegmentRows segment_rows(double t, double dt, int32_t insert, int i, int S, bool stop) {
  MRS_TG_NO_CONTRACT
  SegmentRows r;
  r.nd = (t > kMinSegmentTime) ? ceil(t / dt) : 0.0;
  if (!(r.nd > 0.0)) r.nd = 0.0;  // (t > 0.1 and dt > 0 leave nothing else; a NaN quotient counts as no rows)
  const bool any = r.nd > 0.0;
  r.dwell = (any && i > 0 && stop) ? insert : 0;
  const double clamped = r.nd < kCountClamp ? r.nd : kCountClamp;
  r.rows = (long long)clamped + (long long)(any && i == S - 1) + (long long)r.dwell;
  return r;
}

// the interpolation coefficient of row r (0-based inside its segment)
MRS_TG_HD inline double row_coeff(double nd, int32_t dwell, long long r) {
  MRS_TG_NO_CONTRACT
  const double step = 1.0 / nd;
  const long long j = r > (long long)dwell ? r - (long long)dwell : 0;
  return (double)j * step;
}

// the row itself from the segment's two raw waypoint rows
MRS_TG_HD inline void row_at(const double* a, const double* b, double coeff, double* p) {
  MRS_TG_NO_CONTRACT
  MRS_TG_UNROLL
  for (int k = 0; k < 3; ++k) p[k] = a[k] + coeff * (b[k] - a[k]);
  p[3] = wrap_yaw(interp_heading(a[3], b[3], coeff));
}

// a row count or a first row as the outputs report it: itself when it fits, capacity + 1 when it does not (capacity <= kMaxCapacity)
MRS_TG_HD inline int32_t saturated(long long n, int32_t capacity) {
  return n > (long long)capacity ? capacity + 1 : (int32_t)n;
}

// the two addends a row gives its segment's vertices, each one rounding behind the weight's own
MRS_TG_HD inline double towards_b(double coeff, double g) {
  MRS_TG_NO_CONTRACT
  return coeff * g;
}
MRS_TG_HD inline double towards_a(double coeff, double g) {
  MRS_TG_NO_CONTRACT
  const double w = 1.0 - coeff;
  return w * g;
}

// ---- the harness's restatement, one path after the other -------------------------------------------------------------
// count_rows and vertex_gradient below are NOT code the kernels run: the kernels take the counts by a wavefront prefix sum and
// the sums by an eight-lane walk of an LDS tile (mrs_tg_fallback.hip), and share with this file segment_rows, row_coeff, row_at,
// saturated, segment_of_row, towards_a, towards_b and accumulate.  These two are the same rule and the same order of sums written
// serially, for tests/host/fallback_harness.cpp; the GPU tests hold the kernels to their bits.

// phase A, serially: first[i] (64-bit, not saturated), nd[i], dwell[i] of every segment -> the path's row count
MRS_TG_HD inline long long count_rows(const double* seg_times, const uint8_t* stop_at, int S, double dt, int32_t insert,
                                      long long* first, double* nd, int32_t* dwell) {
  long long total = 0;
  for (int i = 0; i < S; ++i) {
    const SegmentRows r = segment_rows(seg_times[i], dt, insert, i, S, stop_at != nullptr && stop_at[i] != 0);
    first[i] = total, nd[i] = r.nd, dwell[i] = r.dwell;
    total += r.rows;
  }
  return total;
}

// the segment of row r: the largest i with first[i] <= r (segments without rows share their successor's first row and lose)
template <class Int>
MRS_TG_HD inline int segment_of_row(const Int* first, int S, long long r) {
  int lo = 0, hi = S;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((long long)first[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// dL/dwaypoint v of a path, [4], in the order stated on top; grad_samples [min(count, capacity)][4] are the path's rows
MRS_TG_HD inline void vertex_gradient(const long long* first, const double* nd, const int32_t* dwell, int S, long long n,
                                      const double* grad_samples, int v, double* g) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int side = 0; side < 2; ++side) {
    const int i = v - 1 + side;  // segment v - 1 gives this vertex `towards_b`, segment v `towards_a`
    if (i < 0 || i >= S) continue;
    const long long r0 = first[i], r1 = i + 1 < S ? first[i + 1] : n;
    for (long long r = r0; r < r1 && r < n; ++r) {
      const double c = row_coeff(nd[i], dwell[i], r - r0);
      for (int k = 0; k < 4; ++k) {
        const double up = grad_samples[(size_t)r * 4 + k];
        acc[k] = accumulate(acc[k], side == 0 ? towards_b(c, up) : towards_a(c, up));
      }
    }
  }
  for (int k = 0; k < 4; ++k) g[k] = acc[k];
}

}  // namespace fbq
}  // namespace mrs_tg

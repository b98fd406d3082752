// mrs_tg_estimate_vjp.hip -- the backward pass of the Euclidean segment-time estimate (mrs_tg_plan_estimate_times_vjp): the
// gradients of a loss L(seg_times) with respect to the waypoints and the limits, and the term every segment's time came from
// (mrs_tg_estimate_vjp.hpp).  One launch, two kinds of lanes.  The first sum V lanes take one vertex
// each: the lane reads its waypoint row and its neighbours', recomputes its at most two segments with the forward's own
// expressions, sums their parts in the header's order and writes its 32-byte gradient row and the term of the segment that
// starts at it.  The n_paths lanes behind them take one path each and sum its segments' limit parts in increasing index into
// the path's nine entries.  Reads only; no atomics, no workspace, every output element written once: two calls give the
// same bits, and a path gives the same bits wherever it sits in the batch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mrs_tg_estimate_vjp.hpp"
#include "mrs_tg_launch.h"

namespace mrs_tg {

static_assert(estvjp::kHorizontal == MRS_TG_ESTIMATE_TERM_HORIZONTAL && estvjp::kVertical == MRS_TG_ESTIMATE_TERM_VERTICAL &&
                  estvjp::kFloor == MRS_TG_ESTIMATE_TERM_FLOOR && estvjp::kHeading == MRS_TG_ESTIMATE_TERM_HEADING,
              "the header's terms are the ABI's");
static_assert(estvjp::kPi == M_PI, "the forward's pi");

namespace {

constexpr int kEvThreads = 256;

}  // namespace

__global__ __launch_bounds__(kEvThreads) void estimate_times_vjp_kernel(BatchView b, const double* __restrict__ wp,
                                                                        const double* __restrict__ limits,
                                                                        const double* __restrict__ grad_times,
                                                                        double* __restrict__ grad_wp,
                                                                        double* __restrict__ grad_limits,
                                                                        int32_t* __restrict__ term) {
  const int n_vertices = b.n_segments + b.n_paths;
  const int idx = (int)blockIdx.x * kEvThreads + (int)threadIdx.x;
  if (idx < n_vertices) {
    if (!grad_wp && !term) return;
    const int v = idx;
    const int p = path_of_vertex(b, v);
    const int seg0 = first_segment(b, p);
    const int S = segments_of(b, p, seg0);
    const int j = v - (seg0 + p);  // the vertex within its path, 0 .. S
    const int own = seg0 + j;      // the segment that starts here (j < S); own - 1 ends here (j > 0)
    const double* lim = limits + (size_t)p * estvjp::kLimits;
    const double* row = wp + (size_t)v * 4;
    const bool has_front = j > 0 && grad_wp, has_own = j < S;
    double g[4];
    int t = estvjp::kFloor;
    estvjp::vertex_gradient(has_front ? row - 4 : nullptr, has_front ? grad_times[own - 1] : 0.0, has_own ? row : nullptr,
                            has_own && grad_wp ? grad_times[own] : 0.0, lim, g, &t);
    if (grad_wp) {
      double* out = grad_wp + (size_t)v * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = g[k];
    }
    if (term && has_own) term[own] = t;
    return;
  }
  const int p = idx - n_vertices;
  if (p >= b.n_paths || !grad_limits) return;
  const int seg0 = first_segment(b, p);
  const int S = segments_of(b, p, seg0);
  double g[estvjp::kLimits];
  estvjp::limit_gradient(wp + (size_t)(seg0 + p) * 4, grad_times + seg0, S, limits + (size_t)p * estvjp::kLimits, g);
  double* out = grad_limits + (size_t)p * estvjp::kLimits;
#pragma unroll
  for (int k = 0; k < estvjp::kLimits; ++k) out[k] = g[k];
}

hipError_t launch_estimate_times_vjp(const BatchView& b, const double* wp, const double* limits, const double* grad_times,
                                     double* grad_wp, double* grad_limits, int32_t* term, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  const long long lanes = (long long)b.n_segments + 2LL * b.n_paths;
  MRS_TG_LAUNCH_TIMED(estimate_times_vjp_kernel, dim3(cdiv(lanes, kEvThreads)), dim3(kEvThreads), 0,
                      stream, b, wp, limits, grad_times, grad_wp, grad_limits, term);
  return hipGetLastError();
}

}  // namespace mrs_tg

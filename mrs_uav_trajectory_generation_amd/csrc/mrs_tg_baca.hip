// mrs_tg_baca.hip -- the Baca segment-time estimate as a plan step (mrs_tg_plan_estimate_times_baca), its backward pass
// (mrs_tg_plan_estimate_times_baca_vjp) and the length gate (mrs_tg_plan_length_gate); mrs_tg_baca.hpp, DESIGN.md section 4f.
// baca_times_kernel: one lane per segment, the lane-to-path map of mrs_tg_batch.hpp; the lane reads rows i - 1 .. i + 2 of
// its own path.  baca_times_vjp_kernel: one launch, two kinds of lanes.  The first sum V lanes take one vertex each: the lane
// recomputes its at most four segments from rows v - 3 .. v + 3 of its own path with the forward's own expressions, sums their
// parts in the header's order and writes its 32-byte gradient row and the flags of the segment that starts at it.  The n_paths
// lanes behind them take one path each and sum its segments' limit parts in increasing index into the path's nine entries.
// length_gate_kernel: one lane per path.  Reads only; no atomics, no workspace, no LDS, every output element written once: two
// calls give the same bits, and a path gives the same bits wherever it sits in the batch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mrs_tg_baca.hpp"
#include "mrs_tg_launch.h"

namespace mrs_tg {

static_assert(baca::kVVertical == MRS_TG_BACA_V_VERTICAL && baca::kAVertical == MRS_TG_BACA_A_VERTICAL &&
                  baca::kJVertical == MRS_TG_BACA_J_VERTICAL && baca::kT1Capped == MRS_TG_BACA_T1_CAPPED &&
                  baca::kT2Capped == MRS_TG_BACA_T2_CAPPED && baca::kDot1Clamped == MRS_TG_BACA_DOT1_CLAMPED &&
                  baca::kDot2Clamped == MRS_TG_BACA_DOT2_CLAMPED && baca::kFloor == MRS_TG_BACA_FLOOR &&
                  baca::kHeading == MRS_TG_BACA_HEADING && baca::kHeadingCruise == MRS_TG_BACA_HEADING_CRUISE &&
                  baca::kHeadingAcc == MRS_TG_BACA_HEADING_ACC,
              "the header's flags are the ABI's");
static_assert(baca::kVerdictAccepted == MRS_TG_FIND_ACCEPTED && baca::kVerdictCode == MRS_TG_FIND_REJECTED_CODE &&
                  baca::kVerdictTooLong == MRS_TG_FIND_REJECTED_TOO_LONG && baca::kVerdictTooShort == MRS_TG_FIND_REJECTED_TOO_SHORT,
              "the gate's verdicts are the ABI's");

namespace {

constexpr int kBacaThreads = 256;

}  // namespace

__global__ __launch_bounds__(kBacaThreads) void baca_times_kernel(BatchView b, const double* __restrict__ wp,
                                                                  const double* __restrict__ limits,
                                                                  double* __restrict__ seg_times) {
  const int idx = (int)blockIdx.x * kBacaThreads + (int)threadIdx.x;
  if (idx >= b.n_segments) return;
  const int p = path_of_segment(b, idx);
  const int seg0 = first_segment(b, p);
  const int S = segments_of(b, p, seg0);
  const double* lim = limits + (size_t)p * baca::kLimits;
  seg_times[idx] = baca::classify(wp + (size_t)(seg0 + p) * 4, idx - seg0, S, lim, baca::thresholds(lim)).value;
}

__global__ __launch_bounds__(kBacaThreads) void baca_times_vjp_kernel(BatchView b, const double* __restrict__ wp,
                                                                      const double* __restrict__ limits,
                                                                      const double* __restrict__ grad_times,
                                                                      double* __restrict__ grad_wp,
                                                                      double* __restrict__ grad_limits,
                                                                      int32_t* __restrict__ flags) {
  const int n_vertices = b.n_segments + b.n_paths;
  const int idx = (int)blockIdx.x * kBacaThreads + (int)threadIdx.x;
  if (idx < n_vertices) {
    if (!grad_wp && !flags) return;
    const int v = idx;
    const int p = path_of_vertex(b, v);
    const int seg0 = first_segment(b, p);
    const int S = segments_of(b, p, seg0);
    const int j = v - (seg0 + p);  // the vertex within its path, 0 .. S
    double g[4];
    int f = baca::kFloor;
    baca::vertex_gradient(wp + (size_t)(seg0 + p) * 4, grad_wp ? grad_times + seg0 : nullptr, j, S,
                          limits + (size_t)p * baca::kLimits, g, flags ? &f : nullptr);
    if (grad_wp) {
      double* out = grad_wp + (size_t)v * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) out[k] = g[k];
    }
    if (flags && j < S) flags[seg0 + j] = f;
    return;
  }
  const int p = idx - n_vertices;
  if (p >= b.n_paths || !grad_limits) return;
  const int seg0 = first_segment(b, p);
  const int S = segments_of(b, p, seg0);
  double g[baca::kLimits];
  baca::limit_gradient(wp + (size_t)(seg0 + p) * 4, grad_times + seg0, S, limits + (size_t)p * baca::kLimits, g);
  double* out = grad_limits + (size_t)p * baca::kLimits;
#pragma unroll
  for (int k = 0; k < baca::kLimits; ++k) out[k] = g[k];
}

__global__ __launch_bounds__(kBacaThreads) void length_gate_kernel(BatchView b, const double* __restrict__ seg_times,
                                                                   const int32_t* __restrict__ n_samples, double dt,
                                                                   double max_factor, double min_factor,
                                                                   const int32_t* __restrict__ status, double* __restrict__ total,
                                                                   int32_t* __restrict__ verdict) {
  const int p = (int)blockIdx.x * kBacaThreads + (int)threadIdx.x;
  if (p >= b.n_paths) return;
  const int seg0 = first_segment(b, p);
  const int S = segments_of(b, p, seg0);
  const baca::Gate g = baca::length_gate(seg_times + seg0, S, n_samples[p], dt, max_factor, min_factor, status ? status + p : nullptr);
  if (total) total[p] = g.total;
  if (verdict) verdict[p] = g.verdict;
}

hipError_t launch_baca_times(const BatchView& b, const double* wp, const double* limits, double* seg_times, hipStream_t stream) {
  if (b.n_segments == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(baca_times_kernel, dim3(cdiv(b.n_segments, kBacaThreads)), dim3(kBacaThreads), 0,
                      stream, b, wp, limits, seg_times);
  return hipGetLastError();
}

hipError_t launch_baca_times_vjp(const BatchView& b, const double* wp, const double* limits, const double* grad_times,
                                 double* grad_wp, double* grad_limits, int32_t* flags, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  const long long lanes = (long long)b.n_segments + 2LL * b.n_paths;
  MRS_TG_LAUNCH_TIMED(baca_times_vjp_kernel, dim3(cdiv(lanes, kBacaThreads)), dim3(kBacaThreads), 0,
                      stream, b, wp, limits, grad_times, grad_wp, grad_limits, flags);
  return hipGetLastError();
}

hipError_t launch_length_gate(const BatchView& b, const double* seg_times, const int32_t* n_samples, double dt, double max_factor,
                              double min_factor, const int32_t* status, double* total, int32_t* verdict, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(length_gate_kernel, dim3(cdiv(b.n_paths, kBacaThreads)), dim3(kBacaThreads), 0,
                      stream, b, seg_times, n_samples, dt, max_factor, min_factor, status, total, verdict);
  return hipGetLastError();
}

}  // namespace mrs_tg

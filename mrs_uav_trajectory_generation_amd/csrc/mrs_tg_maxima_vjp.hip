// mrs_tg_maxima_vjp.hip -- the backward pass of the segment maxima (mrs_tg_plan_segment_maxima_vjp): for every segment, the
// gradients of a loss L(maxima) with respect to the coefficients and the segment time (mrs_tg_maxima_vjp.hpp, DESIGN.md
// section 4d).  A workgroup takes kMvSegs segments in the forward's layout: one wavefront per entry (k, group), one lane per
// segment.  Each lane runs the forward's own search with the winner tracked (segment_maximum<1, true>, the numbers of
// segment_maxima9_kernel), refines the winner and leaves the entry's terms in LDS; then the workgroup sums the nine entries of
// each segment in a fixed order and writes the segments' 40 coefficient gradients, times and t* coalesced.  Reads only; no
// atomics, no workspace, every output element written once: two calls give the same bits.
#include <hip/hip_runtime.h>

#include "mrs_tg_launch.h"
#include "mrs_tg_maxima.hpp"
#include "mrs_tg_maxima_vjp.hpp"

namespace mrs_tg {

namespace {

constexpr int kMvSegs = 64;
constexpr int kMvThreads = kMvSegs * maxvjp::kEntries;  // nine wavefronts

}  // namespace

__global__ __launch_bounds__(kMvThreads) void segment_maxima_vjp_kernel(int n_segments, const double* __restrict__ coeffs,
                                                                        const double* __restrict__ seg_times,
                                                                        const double* __restrict__ grad_maxima,
                                                                        double* __restrict__ grad_coeffs,
                                                                        double* __restrict__ grad_times,
                                                                        double* __restrict__ argmax) {
  __shared__ maxvjp::EntryTerms terms[maxvjp::kEntries][kMvSegs];
  __shared__ int usable[maxvjp::kEntries][kMvSegs];
  const int which = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
  const int s0 = (int)blockIdx.x * kMvSegs;
  const int nseg = min(kMvSegs, n_segments - s0);
  if (lane < nseg) {
    const int s = s0 + lane;
    const double* c = coeffs + (size_t)s * kD * kN;
    const double T = seg_times[s];
    const bool ok = maxvjp::entry_valid(c, T, which);
    maxvjp::EntryTerms e{0.0, 0.0, 0.0, 0.0};
    if (ok) {
      ArgmaxOut am;
      (void)segment_maximum<1, true>(c, T, which, 0, &am);
      e = maxvjp::entry_terms(c, T, which, am.tau, am.lo, am.hi, grad_maxima[(size_t)s * maxvjp::kEntries + which]);
    }
    terms[which][lane] = e;
    usable[which][lane] = ok ? 1 : 0;
  }
  __syncthreads();
  // a segment is used only if all nine entries are (together they read every coefficient): otherwise zero rows
  auto seg_ok = [&](int sl) {
    int ok = 1;
#pragma unroll
    for (int w = 0; w < maxvjp::kEntries; ++w) ok &= usable[w][sl];
    return ok != 0;
  };
  if (grad_coeffs) {
    for (int e = (int)threadIdx.x; e < nseg * kD * kN; e += kMvThreads) {
      const int sl = e / (kD * kN), r = e - sl * (kD * kN);
      grad_coeffs[(size_t)s0 * kD * kN + e] = seg_ok(sl) ? maxvjp::coeff_gradient(&terms[0][sl], kMvSegs, r / kN, r % kN) : 0.0;
    }
  }
  if (argmax) {
    for (int e = (int)threadIdx.x; e < nseg * maxvjp::kEntries; e += kMvThreads) {
      const int sl = e / maxvjp::kEntries, w = e - sl * maxvjp::kEntries;
      argmax[(size_t)s0 * maxvjp::kEntries + e] = seg_ok(sl) ? terms[w][sl].t : 0.0;
    }
  }
  if (grad_times && (int)threadIdx.x < nseg) {
    const int sl = (int)threadIdx.x;
    grad_times[s0 + sl] = seg_ok(sl) ? maxvjp::time_gradient(&terms[0][sl], kMvSegs) : 0.0;
  }
}

hipError_t launch_segment_maxima_vjp(int n_segments, const double* coeffs, const double* seg_times, const double* grad_maxima,
                                     double* grad_coeffs, double* grad_times, double* argmax, hipStream_t stream) {
  if (n_segments <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(segment_maxima_vjp_kernel, dim3(cdiv(n_segments, kMvSegs)), dim3(kMvThreads), 0, stream, n_segments,
                      coeffs, seg_times, grad_maxima, grad_coeffs, grad_times, argmax);
  return hipGetLastError();
}

}  // namespace mrs_tg

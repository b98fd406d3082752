// mrs_tg_vjp.hip -- the backward pass of the fixed-times solve (mrs_tg_plan_solve_vjp): for every path with status > 0, the
// gradients of a loss L(coeffs, cost) with respect to the fixed values and the segment times, by the exact chain rule of the
// linear QP at the returned solution (mrs_tg_vjp.hpp).  Reads fixed_mask, fixed_values, seg_times,
// coeffs, status and the upstream gradients; writes only the two gradient arrays.  One lane per (path, dimension), the four
// lanes of a path in one quad; per-lane factors (L, W, z) in the plan's workspace, element-major so that a wavefront's
// accesses coalesce.  No atomics: a segment's time gradient is summed over the quad in a fixed order, so two calls give the
// same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mrs_tg_device.hpp"
#include "mrs_tg_vjp.hpp"

namespace mrs_tg {

size_t vjp_workspace_doubles(const BatchView& b) {
  return (size_t)(b.max_segments + 1) * vjp::kWsPerVertex * 4 * (size_t)b.n_paths;
}

namespace {

// a segment's time gradient: (dim 0 + dim 1) + (dim 2 + dim 3), written by dimension 0 (addition commutes bit for bit, so
// every lane of the quad holds the same sum)
struct QuadTimeSink {
  double* out;  // the path's first segment, or NULL
  int dim;
  __device__ void operator()(int i, double x) const {
    x = x + __shfl_xor(x, 1, 64);
    x = x + __shfl_xor(x, 2, 64);
    if (dim == 0 && out) out[i] = x;
  }
};

}  // namespace

__global__ __launch_bounds__(64) void vjp_kernel(BatchView b, int d, const uint8_t* __restrict__ mask,
                                                 const double* __restrict__ vals, const double* __restrict__ seg_times,
                                                 const double* __restrict__ coeffs, const int32_t* __restrict__ status,
                                                 const double* __restrict__ grad_coeffs, const double* __restrict__ grad_cost,
                                                 double* __restrict__ ws, double* __restrict__ grad_vals,
                                                 double* __restrict__ grad_times) {
  const unsigned t = blockIdx.x * 64u + threadIdx.x;
  const int q = (int)(t >> 2), dim = (int)(t & 3u);
  if (q >= b.n_paths) return;
  const PathRef pr = path_at(b, q);
  if (!(status[pr.p] > 0)) {  // (the four lanes of a path agree) zero rows for a path the forward did not solve
    if (grad_vals)
      for (int v = 0; v <= pr.S; ++v)
        for (int k = 0; k < kB; ++k) grad_vals[((size_t)(pr.v0 + v) * kB + k) * kD + dim] = 0.0;
    if (grad_times && dim == 0)
      for (int i = 0; i < pr.S; ++i) grad_times[pr.s0 + i] = 0.0;
    return;
  }
  const double g = grad_cost ? grad_cost[pr.p] : 0.0;
  const vjp::LaneWs w{ws + t, (size_t)b.n_paths * 4};
  vjp::vjp_lane(mask, vals, pr.v0, pr.S, d, dim, seg_times + pr.s0, coeffs + (size_t)pr.s0 * kD * kN,
                grad_coeffs ? grad_coeffs + (size_t)pr.s0 * kD * kN : nullptr, g, w, grad_vals,
                QuadTimeSink{grad_times ? grad_times + pr.s0 : nullptr, dim});
}

hipError_t launch_vjp(const BatchView& b, int d, const uint8_t* mask, const double* vals, const double* seg_times,
                      const double* coeffs, const int32_t* status, const double* grad_coeffs, const double* grad_cost, double* ws,
                      double* grad_vals, double* grad_times, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  const unsigned grid = cdiv((long long)b.n_paths * 4, 64);
  MRS_TG_LAUNCH_TIMED(vjp_kernel, dim3(grid), dim3(64), 0, stream, b, d, mask, vals, seg_times, coeffs, status, grad_coeffs,
                      grad_cost, ws, grad_vals, grad_times);
  return hipGetLastError();
}

}  // namespace mrs_tg

// mrs_tg_refine.hip -- the refinement pass of MRS_TG_FLAG_REFINE: a post-pass over a solve's outputs that takes every path
// with status > 0 to the solution of its linear QP at the returned segment times, to about 1e-11 and better where the double
// solve left cond(R_pp) * eps (mrs_tg_refine.hpp: double-double residual, correction solved in double, guarded steps).
// Reads fixed_mask, fixed_values, seg_times and coeffs; rewrites coeffs and cost; never touches seg_times or status.
// One lane per (path, dimension), the four lanes of a path in one quad; per-lane state (factors, iterates) in the plan's
// workspace, element-major so that a wavefront's accesses coalesce.  No atomics: the cost is summed over the quad in a fixed
// order, so two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mrs_tg_device.hpp"
#include "mrs_tg_refine.hpp"

namespace mrs_tg {

size_t refine_workspace_doubles(const BatchView& b) {
  return (size_t)(b.max_segments + 1) * refine::kWsPerVertex * 4 * (size_t)b.n_paths;
}

__global__ __launch_bounds__(64) void refine_kernel(BatchView b, int d, const uint8_t* __restrict__ mask,
                                                    const double* __restrict__ vals, const double* __restrict__ seg_times,
                                                    double* __restrict__ ws, double* __restrict__ coeffs,
                                                    const int32_t* __restrict__ status, double* __restrict__ cost) {
  const unsigned t = blockIdx.x * 64u + threadIdx.x;
  const int q = (int)(t >> 2), dim = (int)(t & 3u);
  if (q >= b.n_paths) return;
  const PathRef pr = path_at(b, q);
  if (!(status[pr.p] > 0)) return;  // (the four lanes of a path agree)
  const refine::LaneWs w{ws + t, (size_t)b.n_paths * 4};
  refine::dd c{0.0, 0.0};
  refine::refine_lane(mask, vals, pr.v0, pr.S, d, dim, seg_times + pr.s0, coeffs + (size_t)pr.s0 * kD * kN, w, c);
  // the path's cost: (dim 0 + dim 1) + (dim 2 + dim 3) in double-double, the same order on every call
  refine::dd o{__shfl_xor(c.hi, 1, 64), __shfl_xor(c.lo, 1, 64)};
  c = (dim & 1) ? refine::dd_add(o, c) : refine::dd_add(c, o);
  o = refine::dd{__shfl_xor(c.hi, 2, 64), __shfl_xor(c.lo, 2, 64)};
  c = (dim & 2) ? refine::dd_add(o, c) : refine::dd_add(c, o);
  if (dim == 0 && cost) cost[pr.p] = c.hi + c.lo;
}

hipError_t launch_refine(const BatchView& b, int d, const uint8_t* mask, const double* vals, const double* seg_times, double* ws,
                         double* coeffs, const int32_t* status, double* cost, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  const unsigned grid = cdiv((long long)b.n_paths * 4, 64);
  MRS_TG_LAUNCH(refine_kernel, dim3(grid), dim3(64), 0, stream, b, d, mask, vals, seg_times, ws, coeffs, status, cost);
  return hipGetLastError();
}

}  // namespace mrs_tg

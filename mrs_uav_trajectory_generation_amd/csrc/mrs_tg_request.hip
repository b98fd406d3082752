// mrs_tg_request.hip -- the request's vertices and limits as plan steps (mrs_tg_request.hpp):
// mrs_tg_plan_request_vertices, mrs_tg_plan_request_limits and their backward passes.
//   request_vertices_kernel      ONE WAVEFRONT PER PATH, one lane one vertex of a chunk of 64.  A chunk's rows are loaded, then
//                                the chain h_i = unwrap(raw_i, h_{i-1}) runs as a wave-uniform loop over the chunk's vertices:
//                                step i reads lane i's raw heading by a uniform-index read, every lane computes the same
//                                fbq::unwrap against the uniform `last`, lane i keeps the result; the last value carries into
//                                the next chunk.  Each lane then writes its own vertex: the waypoint row, the 5 mask bytes, the
//                                20 values as ten 16-byte words.  waypoints_out may be waypoints: a lane reads its row before it
//                                writes it, and a chunk reads only its own rows.
//   request_vertices_vjp_kernel  one lane per vertex: its row of grad_waypoints; the lane of a path's first vertex also writes
//                                that path's state block.
//   request_limits_kernel, request_limits_vjp_kernel   one lane per path.
// No LDS, no atomics, no workspace; no workgroup waits for another.  Every output element a step owns is written exactly once,
// zeros included.
#include <hip/hip_runtime.h>

#include "../../include/mrs_tg.h"
#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"
#include "mrs_tg_request.hpp"

namespace mrs_tg {

static_assert(reqq::kReqOverride == MRS_TG_REQ_OVERRIDE && reqq::kReqRelaxHeading == MRS_TG_REQ_RELAX_HEADING &&
                  reqq::kOverridden == MRS_TG_LIM_OVERRIDDEN && reqq::kOverrideRefused == MRS_TG_LIM_OVERRIDE_REFUSED &&
                  reqq::kRelaxed == MRS_TG_LIM_RELAXED && reqq::kVDescending == MRS_TG_LIM_V_DESCENDING &&
                  reqq::kADescending == MRS_TG_LIM_A_DESCENDING && reqq::kJDescending == MRS_TG_LIM_J_DESCENDING &&
                  reqq::kFallback == MRS_TG_LIM_FALLBACK,
              "the flags and the branch word of the header are the ABI's");
static_assert(reqq::kChunk == 64, "one lane per vertex of a chunk");

namespace {

constexpr int kLaneThreads = 256;

__device__ __forceinline__ void store_pairs(double* to, const double* from, int n_pairs) {
  row_pair* out = reinterpret_cast<row_pair*>(to);
  for (int e = 0; e < n_pairs; ++e) {
    row_pair w;
    w.x = from[2 * e], w.y = from[2 * e + 1];
    out[e] = w;
  }
}

}  // namespace

// (waypoints_out may be waypoints)
__global__ __launch_bounds__(64) void request_vertices_kernel(BatchView b, const double* waypoints,
                                                              const uint8_t* __restrict__ stop_at,
                                                              const uint8_t* __restrict__ has_state,
                                                              const double* __restrict__ state, int d, double* waypoints_out,
                                                              uint8_t* __restrict__ mask, double* __restrict__ vals) {
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int V = pr.S + 1;
  const bool has = has_state != nullptr && has_state[pr.p] != 0;
  const double* __restrict__ st = state + (size_t)pr.p * reqq::kState;  // (read only where the path has a state)
  const double* rows = waypoints + (size_t)pr.v0 * 4;
  double last = has ? st[3] : rows[3];
  for (int c0 = 0; c0 < V; c0 += reqq::kChunk) {
    const int i = c0 + lane;
    double w[kD] = {0.0, 0.0, 0.0, 0.0};
    if (i < V) {
      const row_pair* r = reinterpret_cast<const row_pair*>(rows + (size_t)i * 4);
      const row_pair lo = r[0], hi = r[1];
      w[0] = lo.x, w[1] = lo.y, w[2] = hi.x, w[3] = hi.y;
    }
    const double raw = w[3];
    const int n = min(reqq::kChunk, V - c0);
    for (int k = 0; k < n; ++k) {  // the chain: wave-uniform, `last` the same in every lane
      last = fbq::unwrap(lane_value(raw, k), last);
      if (lane == k) w[3] = last;
    }
    if (i >= V) continue;
    const size_t v = (size_t)pr.v0 + i;
    if (waypoints_out) store_pairs(waypoints_out + v * 4, w, 2);
    if (mask) {
      uint8_t m[kB];
      reqq::vertex_mask(i == 0, i == V - 1, has, stop_at != nullptr && stop_at[v] != 0, d, m);
#pragma unroll
      for (int k = 0; k < kB; ++k) mask[v * kB + k] = m[k];
    }
    if (vals) {
      double val[reqq::kVertexValues];
      reqq::vertex_values(w, i == 0 && has, st, val);
      row_pair* out = reinterpret_cast<row_pair*>(vals + v * reqq::kVertexValues);
#pragma unroll
      for (int e = 0; e < reqq::kVertexValues / 2; ++e) {
        row_pair q;
        q.x = val[2 * e], q.y = val[2 * e + 1];
        out[e] = q;
      }
    }
  }
}

__global__ __launch_bounds__(kLaneThreads) void request_vertices_vjp_kernel(BatchView b, const uint8_t* __restrict__ has_state,
                                                                            const double* __restrict__ grad_wp,
                                                                            const double* __restrict__ grad_vals,
                                                                            double* __restrict__ grad_raw,
                                                                            double* __restrict__ grad_state) {
  const int v = blockIdx.x * kLaneThreads + threadIdx.x;
  if (v >= b.n_segments + b.n_paths) return;
  const double* gv = grad_vals ? grad_vals + (size_t)v * reqq::kVertexValues : nullptr;
  if (grad_raw) {
    double g[kD];
    reqq::vertex_vjp(grad_wp ? grad_wp + (size_t)v * 4 : nullptr, gv, g);
    store_pairs(grad_raw + (size_t)v * 4, g, 2);
  }
  if (!grad_state) return;
  const int p = path_of_vertex(b, v);
  if (v != first_vertex(b, p)) return;
  double gs[reqq::kState];
  reqq::state_vjp(has_state != nullptr && has_state[p] != 0, gv, gs);
  store_pairs(grad_state + (size_t)p * reqq::kState, gs, reqq::kState / 2);
}

__global__ __launch_bounds__(kLaneThreads) void request_limits_kernel(int n_paths, const double* __restrict__ constraints,
                                                                      const double* __restrict__ override_,
                                                                      const int32_t* __restrict__ flags,
                                                                      const uint8_t* __restrict__ has_state,
                                                                      const double* __restrict__ state, int fallback,
                                                                      double speed_factor, double accel_factor,
                                                                      double* __restrict__ limits, int32_t* __restrict__ branch) {
  const int p = blockIdx.x * kLaneThreads + threadIdx.x;
  if (p >= n_paths) return;
  double c[reqq::kConstraints], o[reqq::kOverrides], lim[reqq::kLimits];
#pragma unroll
  for (int e = 0; e < reqq::kConstraints; ++e) c[e] = constraints[(size_t)p * reqq::kConstraints + e];
  const int32_t f = flags ? flags[p] : 0;
#pragma unroll
  for (int e = 0; e < reqq::kOverrides; ++e) o[e] = (f & reqq::kReqOverride) ? override_[(size_t)p * reqq::kOverrides + e] : 0.0;
  const bool has = has_state != nullptr && has_state[p] != 0;
  const int32_t word = reqq::limits(c, o, f, has, state + (size_t)p * reqq::kState, fallback != 0, speed_factor, accel_factor, lim);
  if (limits) {
#pragma unroll
    for (int k = 0; k < reqq::kLimits; ++k) limits[(size_t)p * reqq::kLimits + k] = lim[k];
  }
  if (branch) branch[p] = word;
}

__global__ __launch_bounds__(kLaneThreads) void request_limits_vjp_kernel(int n_paths, const int32_t* __restrict__ branch,
                                                                          int fallback, double speed_factor, double accel_factor,
                                                                          const double* __restrict__ grad_limits,
                                                                          double* __restrict__ grad_constraints,
                                                                          double* __restrict__ grad_override) {
  const int p = blockIdx.x * kLaneThreads + threadIdx.x;
  if (p >= n_paths) return;
  double g[reqq::kLimits], gc[reqq::kConstraints], go[reqq::kOverrides];
#pragma unroll
  for (int k = 0; k < reqq::kLimits; ++k) g[k] = grad_limits[(size_t)p * reqq::kLimits + k];
  reqq::limits_vjp(branch[p], fallback != 0, speed_factor, accel_factor, g, gc, go);
  if (grad_constraints) store_pairs(grad_constraints + (size_t)p * reqq::kConstraints, gc, reqq::kConstraints / 2);
  if (grad_override) store_pairs(grad_override + (size_t)p * reqq::kOverrides, go, reqq::kOverrides / 2);
}

hipError_t launch_request_vertices(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const uint8_t* has_state,
                                   const double* state, int d, double* waypoints_out, uint8_t* mask, double* vals,
                                   hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(request_vertices_kernel, dim3((unsigned)b.n_paths), dim3(64), 0, stream, b, waypoints, stop_at, has_state,
                      state, d, waypoints_out, mask, vals);
  return hipGetLastError();
}

hipError_t launch_request_vertices_vjp(const BatchView& b, const uint8_t* has_state, const double* grad_wp, const double* grad_vals,
                                       double* grad_raw, double* grad_state, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(request_vertices_vjp_kernel, dim3(cdiv((long long)b.n_segments + b.n_paths, kLaneThreads)),
                      dim3(kLaneThreads), 0, stream, b, has_state, grad_wp, grad_vals, grad_raw, grad_state);
  return hipGetLastError();
}

hipError_t launch_request_limits(int n_paths, const double* constraints, const double* override_, const int32_t* flags,
                                 const uint8_t* has_state, const double* state, int fallback, double speed_factor,
                                 double accel_factor, double* limits, int32_t* branch, hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(request_limits_kernel, dim3(cdiv(n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream, n_paths, constraints,
                      override_, flags, has_state, state, fallback, speed_factor, accel_factor, limits, branch);
  return hipGetLastError();
}

hipError_t launch_request_limits_vjp(int n_paths, const int32_t* branch, int fallback, double speed_factor, double accel_factor,
                                     const double* grad_limits, double* grad_constraints, double* grad_override,
                                     hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(request_limits_vjp_kernel, dim3(cdiv(n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream, n_paths, branch,
                      fallback, speed_factor, accel_factor, grad_limits, grad_constraints, grad_override);
  return hipGetLastError();
}

}  // namespace mrs_tg

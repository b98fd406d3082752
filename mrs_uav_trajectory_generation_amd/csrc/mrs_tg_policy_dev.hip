// mrs_tg_policy_dev.hip -- the policy layer's per-round work that scales with the batch, on the device (round 6).
//
// MrsTrajectoryGeneration::optimize() (/root/reference/src/mrs_trajectory_generation.cpp:620-851) re-solves a request up to seven
// times; around every solve it builds the vertices (:923-977) and scans the sampled trajectory against the waypoint polyline
// (validateTrajectorySpatial, :1401-1455).  For a batch of requests the host used to build [vertex][5][4] value arrays that
// are 80 % zeros, send them up, bring every path's samples down, and scan them on 16 threads: 19-24 of the 51 ms of 4096
// requests were those transfers, 13 the scans.  Here
//   policy_expand_kernel    one lane per VERTEX: constraint mask and values from (unwrapped waypoint, flags, initial state);
//                           what travels up is 36 bytes per vertex instead of 197;
//   policy_validate_kernel  one lane per PATH: the nodelet's gate on the optimiser's code (:1138-1149), the length check
//                           against the Baca total (:1178-1199), then validateTrajectorySpatial as written -- a sequential
//                           scan with a waypoint cursor -- on the samples where they are; what travels down is a few words
//                           per path, one byte per segment, and the samples of the paths that are FINISHED.
// The mask and the values are reqq::vertex_mask and reqq::vertex_values (mrs_tg_request.hpp), the gates are baca::code_accepted
// and baca::length_check (mrs_tg_baca.hpp) and the scan is devq::validate (mrs_tg_deviation.hpp): the functions the host route
// of mrs_tg_policy_host.hpp calls, contraction off, so the vertices are the same bytes and the decisions
// `distance > max_deviation` and the reported maximum are the same bits on both routes (tests/test_gpu_policy.py compares them).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mrs_tg_launch.h"
#include "mrs_tg_policy_host.hpp"

namespace mrs_tg {

// vinfo[v] = path index (position in the round's batch) << 4 | flags; init [path][4][4], the state rows reqq reads
__global__ __launch_bounds__(256) void policy_expand_kernel(int n_vertices, int d, const double* __restrict__ wp,
                                                            const int32_t* __restrict__ vinfo, const double* __restrict__ init,
                                                            uint8_t* __restrict__ mask, double* __restrict__ vals) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_vertices) return;
  const int info = vinfo[v];
  const int a = info >> 4;
  const bool first = info & kVertexFirst, last = info & kVertexLast, stop = info & kVertexStop, has_init = info & kVertexInit;
  double w[kD];
#pragma unroll
  for (int k = 0; k < kD; ++k) w[k] = wp[(size_t)v * 4 + k];
  uint8_t m[kB];
  double val[reqq::kVertexValues];
  reqq::vertex_mask(first, last, has_init, stop, d, m);
  reqq::vertex_values(w, first && has_init, init + (size_t)a * reqq::kState, val);
#pragma unroll
  for (int k = 0; k < 5; ++k) mask[(size_t)v * 5 + k] = m[k];
  double2* out = reinterpret_cast<double2*>(vals + (size_t)v * 20);
#pragma unroll
  for (int e = 0; e < 10; ++e) out[e] = make_double2(val[2 * e], val[2 * e + 1]);
}

__global__ __launch_bounds__(64) void policy_validate_kernel(PolicyValidateArgs g) {
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= g.n_paths) return;
  const int s0 = g.seg_offsets[a], S = g.seg_offsets[a + 1] - s0;
  const int ns = g.n_samples[a], st = g.status[a];
  const bool ok = baca::code_accepted(st) && baca::length_check(ns, g.dt, g.baca_total[a], g.max_len_factor, g.min_len_factor) == 0 &&
                  ns <= g.capacity;
  devq::Validation v;
  v.is_safe = true, v.max_deviation = 0.0;
  if (ok && !g.last_round)  // (the last re-solve is not validated again, :729)
    v = devq::validate(g.samples + (size_t)a * g.capacity * 4, ns, g.wp + (size_t)(s0 + a) * 4, S + 1, g.first_segment,
                       g.max_deviation, g.safe_out + s0);
  const bool is_safe = v.is_safe;
  const bool done = !ok || g.last_round || !(g.check_enabled && !is_safe);
  g.ok_out[a] = ok ? 1 : 0;
  g.ns_out[a] = ns;
  g.status_out[a] = st;
  g.max_dev_out[a] = v.max_deviation;
  g.is_safe_out[a] = is_safe ? 1 : 0;
  g.ns_copy[a] = (ok && done) ? (ns < g.capacity ? ns : g.capacity) : 0;  // rows that travel: the finished paths' samples
}

hipError_t launch_policy_expand(int n_vertices, int d, const double* wp, const int32_t* vinfo, const double* init, uint8_t* mask,
                                double* vals, hipStream_t stream) {
  if (n_vertices <= 0) return hipSuccess;
  MRS_TG_LAUNCH(policy_expand_kernel, dim3(cdiv(n_vertices, 256)), dim3(256), 0, stream, n_vertices, d, wp, vinfo, init,
                mask, vals);
  return hipGetLastError();
}

hipError_t launch_policy_validate(const PolicyValidateArgs& args, hipStream_t stream) {
  if (args.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH(policy_validate_kernel, dim3(cdiv(args.n_paths, 64)), dim3(64), 0, stream, args);
  return hipGetLastError();
}

}  // namespace mrs_tg

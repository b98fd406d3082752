// mrs_tg_passage.hip -- where the sampled trajectory passes the requested waypoints (mrs_tg_plan_waypoint_passage) and its
// backward pass (mrs_tg_plan_waypoint_passage_vjp); mrs_tg_passage.hpp, DESIGN.md section 11c.  The scan is
// getWaypointInTrajectoryIdxs': a waypoint cursor that moves on when a step of the trajectory comes within 0.1 of the waypoint
// at it.  ONE WAVEFRONT TAKES ONE PATH, ONE LANE ONE STEP of a chunk of 64.  The cursor is the only serial part; a chunk
// resolves it by ballots (resolve_hits): all open lanes test the wavefront-uniform waypoint, the first lane that hits records
// it and closes the lanes up to and including itself, the cursor moves on, the lanes behind test again -- hits + 1 rounds of
// one distance per chunk.  Only the waypoint at the cursor and the one behind it are held (fetched one ahead): nothing is
// staged in LDS, W has no upper bound.  A path is finished once the cursor reaches W: its remaining chunks are not loaded.
//   waypoint_passage_kernel      a lane that hit stores index, miss and fraction of its waypoint; the waypoints from the
//                                first one not reached on get -1 / 0.0 behind the loop.
//   waypoint_passage_vjp_kernel  resolves the same hits, fetches the two upstreams of a lane's waypoint, forms the hit's three
//                                rows in its lane, stores the waypoint's and sums a sample row from the lane in front (the
//                                b-part, across a seam in a wavefront-uniform register) and its own a-part.
// A chunk's global loads -- the next chunk's samples, whose first is lane 63's neighbour: the seam -- are issued in front of
// the rounds' arithmetic and of the chunk's stores (rule 1: on gfx950 loads and stores retire through
// one counter).  Reads only; no atomics, no workspace, no LDS; every output element written once.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_passage.hpp"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

namespace {

// what a path's call is about: its samples, its waypoints (wp: row 0 is w_0), their number
struct PassagePath {
  int p, n, W;
  size_t row0, w0;
};

__device__ __forceinline__ PassagePath passage_path(const BatchView& b, const int32_t* __restrict__ n_samples, int capacity,
                                                    const int32_t* __restrict__ wp_offsets, const int32_t* __restrict__ status) {
  const PathRef pr = path_at(b, blockIdx.x);
  PassagePath pp;
  pp.p = pr.p;
  pp.n = live_samples(path_live(status, pr.p), n_samples, pr.p, capacity);
  int w0 = pr.v0, W = pr.S + 1;
  if (wp_offsets) {
    w0 = wp_offsets[pr.p];
    W = wp_offsets[pr.p + 1] - w0;
  }
  pp.W = W < 0 ? 0 : W;
  pp.w0 = (size_t)w0;
  pp.row0 = (size_t)pr.p * (size_t)capacity;
  return pp;
}

// a lane's hit: the waypoint (-1: none), its distance and foot point, its coordinates
struct Hit {
  int k;
  double m, tau, w[3];
};

// The hits of a chunk.  c: the cursor at the chunk's first step, wavefront-uniform, c < W; on return the cursor at the next
// chunk's first step.  wc, wn: the waypoints c and c + 1 (zeros from W on), moved on with the cursor.  open: whether the lane
// holds a step of the scan (i < n - 1).
__device__ __forceinline__ Hit resolve_hits(const double* __restrict__ wp, int W, const double (&s)[3], const double (&nx)[3],
                                            bool open, int lane, int& c, double (&wc)[3], double (&wn)[3]) {
  Hit h;
  h.k = -1;
  h.m = h.tau = h.w[0] = h.w[1] = h.w[2] = 0.0;
  while (c < W && __ballot(open) != 0) {
    const double m = devq::dist(wc, s, nx);
    const double tau = passq::fraction(wc, s, nx);
    const unsigned long long hits = __ballot(open && m < passq::kPassDistance);
    if (hits == 0) break;
    const int f = __ffsll((long long)hits) - 1;
    if (lane == f) {
      h.k = c;
      h.m = m;
      h.tau = tau;
#pragma unroll
      for (int k = 0; k < 3; ++k) h.w[k] = wc[k];
    }
    open = open && lane > f;
    ++c;
#pragma unroll
    for (int k = 0; k < 3; ++k) wc[k] = wn[k];
    load_xyz(wp, c + 1, W, wn);
  }
  return h;
}

}  // namespace

__global__ __launch_bounds__(64) void waypoint_passage_kernel(BatchView b, const double* __restrict__ samples,
                                                              const int32_t* __restrict__ n_samples, int capacity,
                                                              const int32_t* __restrict__ wp_offsets,
                                                              const double* __restrict__ waypoints,
                                                              const int32_t* __restrict__ status, int32_t* __restrict__ index,
                                                              int32_t* __restrict__ count, double* __restrict__ miss,
                                                              double* __restrict__ fraction) {
  const int lane = threadIdx.x;
  const PassagePath pp = passage_path(b, n_samples, capacity, wp_offsets, status);
  const int n = pp.n, W = pp.W;
  const double* __restrict__ rows = samples + pp.row0 * 4;
  const double* __restrict__ wp = waypoints + pp.w0 * 4;
  const bool scans = n > 1 && W > 0;
  double cur[3], wc[3], wn[3];
  load_xyz(rows, lane, scans ? n : 0, cur);
  load_xyz(wp, 0, scans ? W : 0, wc);
  load_xyz(wp, 1, scans ? W : 0, wn);
  int c = 0;
  for (int k0 = 0; scans && k0 < n - 1 && c < W; k0 += 64) {
    const int i = k0 + lane;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    seam_neighbour(cur, nxt, lane, nx);
    const Hit h = resolve_hits(wp, W, cur, nx, i < n - 1, lane, c, wc, wn);
    if (h.k >= 0) {
      if (index) index[pp.w0 + h.k] = i;
      if (miss) miss[pp.w0 + h.k] = h.m;
      if (fraction) fraction[pp.w0 + h.k] = h.tau;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  for (int k = c + lane; k < W; k += 64) {
    if (index) index[pp.w0 + k] = -1;
    if (miss) miss[pp.w0 + k] = 0.0;
    if (fraction) fraction[pp.w0 + k] = 0.0;
  }
  if (count && lane == 0) count[pp.p] = c;
}

__global__ __launch_bounds__(64) void waypoint_passage_vjp_kernel(BatchView b, const double* __restrict__ samples,
                                                                  const int32_t* __restrict__ n_samples, int capacity,
                                                                  const int32_t* __restrict__ wp_offsets,
                                                                  const double* __restrict__ waypoints,
                                                                  const int32_t* __restrict__ status,
                                                                  const double* __restrict__ grad_miss,
                                                                  const double* __restrict__ grad_fraction,
                                                                  double* __restrict__ grad_samples,
                                                                  double* __restrict__ grad_waypoints) {
  const int lane = threadIdx.x;
  const PassagePath pp = passage_path(b, n_samples, capacity, wp_offsets, status);
  const int n = pp.n, W = pp.W;
  const double* __restrict__ rows = samples + pp.row0 * 4;
  const double* __restrict__ wp = waypoints + pp.w0 * 4;
  const bool scans = n > 1 && W > 0;
  double cur[3], wc[3], wn[3];
  load_xyz(rows, lane, scans ? n : 0, cur);
  load_xyz(wp, 0, scans ? W : 0, wc);
  load_xyz(wp, 1, scans ? W : 0, wn);
  int c = 0, k0 = 0;
  // the b-contribution of lane 63's hit, on its way to the next chunk's lane 0 (wavefront-uniform)
  bool carried = false;
  double carry[3] = {0.0, 0.0, 0.0};
  for (; scans && k0 < n && c < W; k0 += 64) {
    const int i = k0 + lane;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    seam_neighbour(cur, nxt, lane, nx);
    const Hit h = resolve_hits(wp, W, cur, nx, i < n - 1, lane, c, wc, wn);
    const bool hit = h.k >= 0;
    // (the upstreams of a waypoint are read once it is known to be reached: those of the others never are)
    const double g_m = hit && grad_miss ? grad_miss[pp.w0 + h.k] : 0.0;
    const double g_t = hit && grad_fraction ? grad_fraction[pp.w0 + h.k] : 0.0;
    double gp[3] = {0.0, 0.0, 0.0}, ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
    if (hit) passq::hit_vjp(h.w, cur, nx, g_m, g_t, gp, ga, gb);
    const unsigned long long hits = __ballot(hit);
    const bool front_hit = lane == 0 ? carried : ((hits >> ((lane + 63) & 63)) & 1ull) != 0;
    double row[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double up = __shfl_up(gb[k], 1);
      const double front = lane == 0 ? carry[k] : up;
      row[k] = 0.0;
      if (front_hit) row[k] = passq::accumulate(row[k], front);
      if (hit) row[k] = passq::accumulate(row[k], ga[k]);
      carry[k] = lane_value(gb[k], 63);
    }
    carried = (hits >> 63) != 0;
    if (grad_samples && i < capacity) store_xyz0(grad_samples + (pp.row0 + i) * 4, row);
    if (grad_waypoints && hit) store_xyz0(grad_waypoints + (pp.w0 + h.k) * 4, gp);
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  row_pair zero;
  zero.x = 0.0, zero.y = 0.0;
  if (grad_samples) {
    // the rows behind the chunks that were run: zeros, but for the row behind a hit on the last lane of the last chunk
    row_pair* out = reinterpret_cast<row_pair*>(grad_samples + pp.row0 * 4);
    for (int e = 2 * k0 + lane; e < 2 * capacity; e += 64) {
      row_pair v = zero;
      if (carried && e == 2 * k0) v.x = passq::accumulate(0.0, carry[0]), v.y = passq::accumulate(0.0, carry[1]);
      if (carried && e == 2 * k0 + 1) v.x = passq::accumulate(0.0, carry[2]);
      out[e] = v;
    }
  }
  if (grad_waypoints) {
    row_pair* out = reinterpret_cast<row_pair*>(grad_waypoints + pp.w0 * 4);
    for (int e = 2 * c + lane; e < 2 * W; e += 64) out[e] = zero;
  }
}

hipError_t launch_waypoint_passage(const BatchView& b, const double* samples, const int32_t* n_samples, int capacity,
                                   const int32_t* wp_offsets, const double* waypoints, const int32_t* status, int32_t* index,
                                   int32_t* count, double* miss, double* fraction, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(waypoint_passage_kernel, dim3((unsigned)b.n_paths), dim3(64), 0, stream, b, samples, n_samples, capacity,
                      wp_offsets, waypoints, status, index, count, miss, fraction);
  return hipGetLastError();
}

hipError_t launch_waypoint_passage_vjp(const BatchView& b, const double* samples, const int32_t* n_samples, int capacity,
                                       const int32_t* wp_offsets, const double* waypoints, const int32_t* status,
                                       const double* grad_miss, const double* grad_fraction, double* grad_samples,
                                       double* grad_waypoints, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(waypoint_passage_vjp_kernel, dim3((unsigned)b.n_paths), dim3(64), 0, stream, b, samples, n_samples,
                      capacity, wp_offsets, waypoints, status, grad_miss, grad_fraction, grad_samples, grad_waypoints);
  return hipGetLastError();
}

}  // namespace mrs_tg

// mrs_tg_obstacle.hip -- how close every row of a batch comes to a static map of obstacles, spheres (x, y, z, radius) or the
// points of a cloud, and which obstacle that is (mrs_tg_plan_obstacle_clearance), and its backward pass
// (mrs_tg_plan_obstacle_clearance_vjp); mrs_tg_obstacle.hpp, DESIGN.md section 11j.  ONE WORKGROUP TAKES ONE PATH, its chunks of
// 64 rows dealt round over the workgroup's wavefronts, ONE LANE ONE ROW OF A CHUNK.
//   obstacle_clearance_kernel      a wavefront takes kObsRows of its chunks at a time: a lane keeps the three coordinates of one row
//                                  of each in registers and walks the obstacles of the path's set once for them, in increasing
//                                  index.  An obstacle's four doubles are the same address for every lane: the index is formed
//                                  from the workgroup's number and from loads through const __restrict__ pointers alone, so the
//                                  loads are scalar loads (one 32-byte load per obstacle and wavefront), kObsUnroll obstacles at a
//                                  time so that they are in flight ahead of their use.  Of those obstacles the squared distances
//                                  are formed first; the square roots are taken only where obsq::cannot_win does not rule all of
//                                  them out for the row -- a wavefront none of whose rows any of them can win on branches round
//                                  the roots, and the header holds the argument why no output bit depends on it.  Every lane
//                                  keeps the first smallest of its rows; write_path_minimum (mrs_tg_pathwave.hpp) combines them
//                                  into the path's minimum.
//   obstacle_clearance_vjp_kernel  one lane per output row: the row, its nearest entry and its upstream, one obstacle loaded where
//                                  the entry names one of the path's own set (obsq::row_gradient).
// Reads only; no atomics, no workspace, no dynamic LDS; every output element written once.  The set's bounds come clamped from
// obsq::path_obstacles, so no index leaves the obstacle array whatever set_offsets, path_set or nearest hold.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_obstacle.hpp"
#include "mrs_tg_pathwave.hpp"

#ifndef MRS_TG_OBSTACLE_WAVES
#define MRS_TG_OBSTACLE_WAVES 4  // wavefronts per workgroup (an experiment build may say 1, 2 or 8: scripts/obstacle_cost.py)
#endif
#ifndef MRS_TG_OBSTACLE_ROWS
#define MRS_TG_OBSTACLE_ROWS 2  // rows a lane keeps across one walk over the obstacles (an experiment build may say 1 or 4)
#endif
#ifndef MRS_TG_OBSTACLE_UNROLL
#define MRS_TG_OBSTACLE_UNROLL 4  // obstacles loaded before the first distance is formed (an experiment build may say 1, 2 or 8)
#endif

namespace mrs_tg {

namespace {

constexpr int kObsWaves = MRS_TG_OBSTACLE_WAVES;
constexpr int kObsThreads = 64 * kObsWaves;
constexpr int kObsUnroll = MRS_TG_OBSTACLE_UNROLL;
constexpr int kObsRows = MRS_TG_OBSTACLE_ROWS;
static_assert(kObsRows >= 1 && kObsRows <= 4, "a lane's rows stay in registers");
static_assert(kObsWaves >= 1 && kObsWaves <= 16, "a workgroup has at most 1024 threads");
static_assert(kObsUnroll >= 1 && kObsUnroll <= 8, "eight obstacles are 64 scalar registers");

}  // namespace

__global__ __launch_bounds__(kObsThreads) void obstacle_clearance_kernel(const double* __restrict__ samples,
                                                                         const int32_t* __restrict__ n_samples, int capacity,
                                                                         const double* __restrict__ obstacles, int n_obstacles,
                                                                         const int32_t* __restrict__ set_offsets, int n_sets,
                                                                         const int32_t* __restrict__ path_set,
                                                                         const int32_t* __restrict__ status, double z_scale,
                                                                         double* __restrict__ clearance,
                                                                         int32_t* __restrict__ nearest,
                                                                         double* __restrict__ min_clearance,
                                                                         int32_t* __restrict__ argmin) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (one value per wavefront: the chunk loop is uniform)
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  const obsq::Bounds ob = obsq::path_obstacles(set_offsets, n_sets, path_set, p, n_obstacles);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  obsq::Nearest best = obsq::nearest_none();  // of this lane's rows: (clearance, row), the first smallest
  int best_nearest = -1;
  for (int k0 = wave * 64; k0 < capacity; k0 += kObsThreads * kObsRows) {
    // the lane's rows of this walk over the obstacles: one of each of the wavefront's next kObsRows chunks
    int r[kObsRows];
    bool mine[kObsRows];  // (a lane behind the path's last row walks along on zeros and takes nothing)
    obsq::Nearest m[kObsRows];
#pragma unroll
    for (int j = 0; j < kObsRows; ++j) r[j] = k0 + j * kObsThreads + lane, mine[j] = r[j] < n, m[j] = obsq::nearest_none();
    if (k0 < n) {
      double cur[kObsRows][3];
#pragma unroll
      for (int j = 0; j < kObsRows; ++j) load_xyz(rows, r[j], n, cur[j]);
      int k = ob.begin;
      for (; ob.end - k >= kObsUnroll; k += kObsUnroll) {
        double o[kObsUnroll][4];
#pragma unroll
        for (int u = 0; u < kObsUnroll; ++u) {
          const double* __restrict__ src = obstacles + (size_t)(k + u) * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[u][e] = src[e];
        }
#pragma unroll
        for (int j = 0; j < kObsRows; ++j) {
          if (k0 + j * kObsThreads >= n) continue;  // (the whole chunk lies behind the path's last row: a wavefront's decision)
          double q[kObsUnroll];
          bool may_win = false;  // any of these against the row's minimum so far (obsq::cannot_win: an older minimum serves)
#pragma unroll
          for (int u = 0; u < kObsUnroll; ++u) {
            q[u] = obsq::distance_squared(cur[j], o[u], z_scale);
            may_win |= !obsq::cannot_win(q[u], m[j].c, o[u][3]);
          }
          if (mine[j] && may_win) {  // (a wavefront none of whose rows they can win on takes no root)
#pragma unroll
            for (int u = 0; u < kObsUnroll; ++u) obsq::take(m[j], obsq::clearance_from(q[u], o[u][3]), k + u);
          }
        }
      }
      for (; k < ob.end; ++k) {
        const double* __restrict__ src = obstacles + (size_t)k * 4;
        const double o[4] = {src[0], src[1], src[2], src[3]};
#pragma unroll
        for (int j = 0; j < kObsRows; ++j)
          if (mine[j]) obsq::take(m[j], obsq::clearance(cur[j], o, z_scale), k);
      }
    }
#pragma unroll
    for (int j = 0; j < kObsRows; ++j) {
      if (r[j] < capacity) {
        if (clearance) clearance[row0 + r[j]] = m[j].c;
        if (nearest) nearest[row0 + r[j]] = m[j].index;
      }
      if (m[j].c < best.c) best.c = m[j].c, best.index = r[j], best_nearest = m[j].index;  // (a lane's rows come in increasing order)
    }
  }
  write_path_minimum<kObsWaves>(best, best_nearest, lane, wave, p, min_clearance, argmin);
}

__global__ __launch_bounds__(kObsThreads) void obstacle_clearance_vjp_kernel(const double* __restrict__ samples,
                                                                             const int32_t* __restrict__ n_samples, int capacity,
                                                                             const double* __restrict__ obstacles, int n_obstacles,
                                                                             const int32_t* __restrict__ set_offsets, int n_sets,
                                                                             const int32_t* __restrict__ path_set,
                                                                             const int32_t* __restrict__ status, double z_scale,
                                                                             const int32_t* __restrict__ nearest,
                                                                             const double* __restrict__ grad_clearance,
                                                                             double* __restrict__ grad_samples) {
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  const obsq::Bounds ob = obsq::path_obstacles(set_offsets, n_sets, path_set, p, n_obstacles);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  for (int r = threadIdx.x; r < capacity; r += kObsThreads) {
    double gi[3] = {0.0, 0.0, 0.0};
    if (r < n) {
      double cur[3];
      load_xyz(rows, r, n, cur);
      obsq::row_gradient(cur, obstacles, ob, nearest[row0 + r], z_scale, grad_clearance[row0 + r], gi);
    }
    store_xyz0(grad_samples + (row0 + r) * 4, gi);  // (rows from n on and a dead path's rows: zeros)
  }
}

hipError_t launch_obstacle_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                     const double* obstacles, int n_obstacles, const int32_t* set_offsets, int n_sets,
                                     const int32_t* path_set, const int32_t* status, double z_scale, double* clearance,
                                     int32_t* nearest, double* min_clearance, int32_t* argmin, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(obstacle_clearance_kernel, dim3((unsigned)n_paths), dim3(kObsThreads), 0, stream, samples, n_samples,
                      capacity, obstacles, n_obstacles, set_offsets, n_sets, path_set, status, z_scale, clearance, nearest,
                      min_clearance, argmin);
  return hipGetLastError();
}

hipError_t launch_obstacle_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                         const double* obstacles, int n_obstacles, const int32_t* set_offsets, int n_sets,
                                         const int32_t* path_set, const int32_t* status, double z_scale, const int32_t* nearest,
                                         const double* grad_clearance, double* grad_samples, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(obstacle_clearance_vjp_kernel, dim3((unsigned)n_paths), dim3(kObsThreads), 0, stream, samples, n_samples,
                      capacity, obstacles, n_obstacles, set_offsets, n_sets, path_set, status, z_scale, nearest, grad_clearance,
                      grad_samples);
  return hipGetLastError();
}

}  // namespace mrs_tg

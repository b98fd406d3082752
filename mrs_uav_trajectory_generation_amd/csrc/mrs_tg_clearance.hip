// mrs_tg_clearance.hip -- how close the paths of one group (a swarm) come to each other, step by step, and who the neighbour is
// (mrs_tg_plan_mutual_clearance), and its backward pass (mrs_tg_plan_mutual_clearance_vjp); mrs_tg_clearance.hpp, DESIGN.md
// section 11i.  ONE WORKGROUP TAKES ONE PATH, its chunks of 64 rows dealt round over the workgroup's wavefronts, ONE LANE ONE ROW.
//   mutual_clearance_kernel      the loop over the group's other paths is the outer loop of a chunk: a neighbour's rows at the
//                                chunk's steps are consecutive, one 16 + 8 byte load per lane, taken kClrUnroll neighbours at a
//                                time so that independent loads are in flight; the distances are then taken in increasing path
//                                index.  Every lane keeps the first smallest of its rows; write_path_minimum
//                                (mrs_tg_pathwave.hpp) combines them into the path's minimum.
//   mutual_clearance_vjp_kernel  a gather: the lane of row (j, r) takes its own term against its own partner, then walks the
//                                group in increasing path index and reads the partner entry of each path's row at the same step
//                                (consecutive int32 across the lanes); the neighbour's row and upstream are loaded only where
//                                the entry names j.
// A path's rows are re-read once per member of its group; those reads are L2 hits (DESIGN.md section 11i has the measurement).
// Reads only; no atomics, no workspace, no dynamic LDS; every output element written once.  The group's bounds come clamped from
// clrq::group_of and every row index from clrq::row_at_step, so no index leaves the plan's arrays whatever group_offsets,
// first_step or partner hold.
#include <hip/hip_runtime.h>

#include "mrs_tg_clearance.hpp"
#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

#ifndef MRS_TG_CLEARANCE_WAVES
#define MRS_TG_CLEARANCE_WAVES 4  // wavefronts per workgroup (an experiment build may say 1, 2 or 8: scripts/clearance_cost.py)
#endif

namespace mrs_tg {

namespace {

constexpr int kClrWaves = MRS_TG_CLEARANCE_WAVES;
constexpr int kClrThreads = 64 * kClrWaves;
constexpr int kClrUnroll = 4;  // neighbours whose rows are loaded before the first distance is formed
static_assert(kClrWaves >= 1 && kClrWaves <= 16, "a workgroup has at most 1024 threads");

// what the kernels know of a path other than their own: its live rows and the step of its row 0
struct PathSpan {
  int n, first;
};
__device__ __forceinline__ PathSpan path_span(const int32_t* __restrict__ status, const int32_t* __restrict__ n_samples,
                                              const int32_t* __restrict__ first_step, int p, int capacity) {
  PathSpan s;
  s.n = live_samples(path_live(status, p), n_samples, p, capacity);
  s.first = first_step ? first_step[p] : 0;
  return s;
}

}  // namespace

__global__ __launch_bounds__(kClrThreads) void mutual_clearance_kernel(int n_paths, const double* __restrict__ samples,
                                                                       const int32_t* __restrict__ n_samples, int capacity,
                                                                       const int32_t* __restrict__ group_offsets, int n_groups,
                                                                       const int32_t* __restrict__ first_step,
                                                                       const int32_t* __restrict__ status, double z_scale,
                                                                       double* __restrict__ clearance,
                                                                       int32_t* __restrict__ partner,
                                                                       double* __restrict__ min_clearance,
                                                                       int32_t* __restrict__ argmin) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x;
  const PathSpan me = path_span(status, n_samples, first_step, p, capacity);
  const int n = me.n;
  const clrq::Bounds gb = clrq::group_of(group_offsets, n_groups, p, n_paths);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  clrq::Nearest best = clrq::nearest_none();  // of this lane's rows: (clearance, row), the first smallest
  int best_partner = -1;
  for (int k0 = wave * 64; k0 < capacity; k0 += kClrThreads) {
    const int r = k0 + lane;
    const bool mine = r < n;
    clrq::Nearest m = clrq::nearest_none();
    if (k0 < n) {
      double cur[3];
      load_xyz(rows, r, n, cur);
      const long long s = clrq::step_of(me.first, r);
      for (int j0 = gb.begin; j0 < gb.end; j0 += kClrUnroll) {
        double v[kClrUnroll][3];
        bool has[kClrUnroll];
#pragma unroll
        for (int u = 0; u < kClrUnroll; ++u) {
          const int j = j0 + u;
          has[u] = false;
          v[u][0] = v[u][1] = v[u][2] = 0.0;
          if (j < gb.end && j != p) {
            const PathSpan o = path_span(status, n_samples, first_step, j, capacity);
            const int rj = clrq::row_at_step(s, o.first, o.n);
            has[u] = mine && rj >= 0;
            if (has[u]) load_xyz(samples + (size_t)j * (size_t)capacity * 4, rj, o.n, v[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < kClrUnroll; ++u)
          if (has[u]) clrq::take(m, clrq::distance(cur, v[u], z_scale), j0 + u);
      }
    }
    if (r < capacity) {
      if (clearance) clearance[row0 + r] = m.c;
      if (partner) partner[row0 + r] = m.index;
    }
    if (m.c < best.c) best.c = m.c, best.index = r, best_partner = m.index;  // (a lane's rows come in increasing order)
  }
  write_path_minimum<kClrWaves>(best, best_partner, lane, wave, p, min_clearance, argmin);
}

__global__ __launch_bounds__(kClrThreads) void mutual_clearance_vjp_kernel(int n_paths, const double* __restrict__ samples,
                                                                           const int32_t* __restrict__ n_samples, int capacity,
                                                                           const int32_t* __restrict__ group_offsets,
                                                                           int n_groups, const int32_t* __restrict__ first_step,
                                                                           const int32_t* __restrict__ status, double z_scale,
                                                                           const int32_t* __restrict__ partner,
                                                                           const double* __restrict__ grad_clearance,
                                                                           double* __restrict__ grad_samples) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x;
  const PathSpan me = path_span(status, n_samples, first_step, p, capacity);
  const int n = me.n;
  const clrq::Bounds gb = clrq::group_of(group_offsets, n_groups, p, n_paths);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  for (int k0 = wave * 64; k0 < capacity; k0 += kClrThreads) {
    const int r = k0 + lane;
    const bool mine = r < n;
    double acc[3] = {0.0, 0.0, 0.0};
    if (k0 < n) {
      double cur[3];
      load_xyz(rows, r, n, cur);
      const long long s = clrq::step_of(me.first, r);
      if (mine) {  // the row's own term, against its own partner
        const int q = partner[row0 + r];
        if (clrq::partner_in_group(q, p, gb)) {
          const PathSpan o = path_span(status, n_samples, first_step, q, capacity);
          const int rq = clrq::row_at_step(s, o.first, o.n);
          if (rq >= 0) {
            double v[3], gi[3];
            load_xyz(samples + (size_t)q * (size_t)capacity * 4, rq, o.n, v);
            clrq::row_vjp(cur, v, z_scale, grad_clearance[row0 + r], gi);
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = clrq::accumulate(acc[k], gi[k]);
          }
        }
      }
      for (int i0 = gb.begin; i0 < gb.end; i0 += kClrUnroll) {  // the rows that name this one, in increasing path index
        int ri[kClrUnroll], ni[kClrUnroll];
        bool names[kClrUnroll];
#pragma unroll
        for (int u = 0; u < kClrUnroll; ++u) {
          const int i = i0 + u;
          names[u] = false;
          ri[u] = -1, ni[u] = 0;
          if (i < gb.end && i != p) {
            const PathSpan o = path_span(status, n_samples, first_step, i, capacity);
            ri[u] = clrq::row_at_step(s, o.first, o.n);
            ni[u] = o.n;
            if (mine && ri[u] >= 0) names[u] = partner[(size_t)i * (size_t)capacity + ri[u]] == p;
          }
        }
#pragma unroll
        for (int u = 0; u < kClrUnroll; ++u) {
          if (!names[u]) continue;
          const size_t at = (size_t)(i0 + u) * (size_t)capacity;
          double v[3], gi[3], gj[3];
          load_xyz(samples + at * 4, ri[u], ni[u], v);
          clrq::row_vjp(v, cur, z_scale, grad_clearance[at + ri[u]], gi);
          clrq::partner_row(gi, gj);
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] = clrq::accumulate(acc[k], gj[k]);
        }
      }
    }
    if (r < capacity) store_xyz0(grad_samples + (row0 + r) * 4, acc);  // (rows from n on and a dead path's rows: zeros)
  }
}

hipError_t launch_mutual_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                   const int32_t* group_offsets, int n_groups, const int32_t* first_step, const int32_t* status,
                                   double z_scale, double* clearance, int32_t* partner, double* min_clearance, int32_t* argmin,
                                   hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(mutual_clearance_kernel, dim3((unsigned)n_paths), dim3(kClrThreads), 0, stream, n_paths, samples, n_samples,
                      capacity, group_offsets, n_groups, first_step, status, z_scale, clearance, partner, min_clearance, argmin);
  return hipGetLastError();
}

hipError_t launch_mutual_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                       const int32_t* group_offsets, int n_groups, const int32_t* first_step,
                                       const int32_t* status, double z_scale, const int32_t* partner, const double* grad_clearance,
                                       double* grad_samples, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(mutual_clearance_vjp_kernel, dim3((unsigned)n_paths), dim3(kClrThreads), 0, stream, n_paths, samples,
                      n_samples, capacity, group_offsets, n_groups, first_step, status, z_scale, partner, grad_clearance,
                      grad_samples);
  return hipGetLastError();
}

}  // namespace mrs_tg

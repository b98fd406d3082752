// mrs_tg_field.hip -- how close every row of a batch comes to a static map given as a voxel grid of signed distances, looked up
// by trilinear interpolation (mrs_tg_plan_field_clearance), and its backward pass (mrs_tg_plan_field_clearance_vjp);
// mrs_tg_field.hpp, DESIGN.md section 11k.  ONE WORKGROUP TAKES ONE PATH, its chunks of 64 rows dealt round over the workgroup's
// wavefronts, ONE LANE ONE ROW OF A CHUNK -- mrs_tg_obstacle.hip's shape, with eight gathered voxels in place of the walk over
// the obstacles.
//   field_clearance_kernel      a wavefront takes kFldRows of its chunks at a time.  A lane locates its rows first (three
//                               divisions and the inside test each: fldq::locate), then loads the eight corners of every one of
//                               them -- 8 kFldRows loads that depend on nothing but the cells, issued before the first is used --
//                               and only then interpolates (fldq::interpolate, and fldq::gradient where the caller wants the
//                               field's gradient).  A lane whose row is not inside or behind the path's last row loads the
//                               first cell of the path's grid instead and drops it, so that no branch keeps the loads apart;
//                               a path without a grid loads nothing.  Every lane keeps the first smallest of its rows;
//                               the path's minimum is combined as write_path_minimum (mrs_tg_pathwave.hpp) does it, by this
//                               kernel's own copy of those lines (DESIGN.md section 4a has the reason).
//   field_clearance_vjp_kernel  one lane per output row: the row, its recorded cell and its upstream; the eight corners are
//                               loaded only where the cell is a low corner of the path's own grid (fldq::row_gradient).
// Reads only; no atomics, no workspace, no dynamic LDS; every output element written once.  A cell the forward forms lies in
// [0, n - 2] on every axis of a grid in [0, n_fields), and the backward pass dereferences a recorded cell only after
// fldq::cell_of_path says the same of it, so no read leaves the fields array whatever path_field and cell hold.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_field.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

#ifndef MRS_TG_FIELD_WAVES
#define MRS_TG_FIELD_WAVES 4  // wavefronts per workgroup (an experiment build may say 1, 2 or 8: scripts/field_cost.py)
#endif
#ifndef MRS_TG_FIELD_ROWS
#define MRS_TG_FIELD_ROWS 2  // rows of a lane whose sixteen voxel loads are in flight together (an experiment build may say 1 or 4)
#endif

namespace mrs_tg {

namespace {

constexpr int kFldWaves = MRS_TG_FIELD_WAVES;
constexpr int kFldThreads = 64 * kFldWaves;
constexpr int kFldRows = MRS_TG_FIELD_ROWS;
static_assert(kFldRows >= 1 && kFldRows <= 4, "a lane's corners stay in registers");
static_assert(kFldWaves >= 1 && kFldWaves <= 16, "a workgroup has at most 1024 threads");

}  // namespace

__global__ __launch_bounds__(kFldThreads) void field_clearance_kernel(const double* __restrict__ samples,
                                                                      const int32_t* __restrict__ n_samples, int capacity,
                                                                      const double* __restrict__ fields, fldq::Geometry G,
                                                                      const int32_t* __restrict__ path_field,
                                                                      const int32_t* __restrict__ status, double outside_value,
                                                                      double* __restrict__ clearance, int32_t* __restrict__ cell_out,
                                                                      double* __restrict__ gradient_out,
                                                                      double* __restrict__ min_clearance,
                                                                      int32_t* __restrict__ argmin) {
  __shared__ double s_c[kFldWaves];
  __shared__ int s_row[kFldWaves], s_cell[kFldWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (one value per wavefront: the chunk loop is uniform)
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  const int f =fldq::grid_of_path(path_field, p, G.n_fields);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  const int first_cell = f >= 0 ? fldq::encode_cell(G, f, 0, 0, 0) : 0;
  fldq::Nearest best = fldq::nearest_none();  // of this lane's rows: (clearance, row), the first smallest
  int best_cell = -1;
  for (int k0 = wave * 64; k0 < capacity; k0 += kFldThreads * kFldRows) {
    int r[kFldRows], cell[kFldRows];
    double c[kFldRows], g[kFldRows][3];
#pragma unroll
    for (int j = 0; j < kFldRows; ++j) {
      r[j] = k0 + j * kFldThreads + lane;
      cell[j] = -1, c[j] = fldq::no_clearance();  // (a path that sees no grid, the rows from n on: +inf / -1)
      g[j][0] = g[j][1] = g[j][2] = 0.0;
    }
    if (f >= 0 && k0 < n) {  // (a wavefront's decision: the path sees a grid and the first of these chunks has a live row)
      double cur[kFldRows][3], t[kFldRows][3], v[kFldRows][8];
#pragma unroll
      for (int j = 0; j < kFldRows; ++j) load_xyz(rows, r[j], n, cur[j]);
#pragma unroll
      for (int j = 0; j < kFldRows; ++j) {
        t[j][0] = t[j][1] = t[j][2] = 0.0;
        if (r[j] < n && !fldq::locate(cur[j], G, f, cell[j], t[j])) c[j] = outside_value;
      }
      // Every corner of every row of the lane, before the first use.  The loads are unconditional so that nothing keeps them
      // apart: a lane without a cell reads the first cell of the path's grid (dims >= 2: its corners exist) and drops it.
#pragma unroll
      for (int j = 0; j < kFldRows; ++j) fldq::load_corners(fields, G, cell[j] >= 0 ? cell[j] : first_cell, v[j]);
#pragma unroll
      for (int j = 0; j < kFldRows; ++j) {
        if (cell[j] >= 0) {
          c[j] = fldq::interpolate(v[j], t[j]);
          if (gradient_out) fldq::gradient(v[j], t[j], G, g[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kFldRows; ++j) {
      if (r[j] < capacity) {
        if (clearance) clearance[row0 + r[j]] = c[j];
        if (cell_out) cell_out[row0 + r[j]] = cell[j];
        if (gradient_out) store_xyz0(gradient_out + (row0 + r[j]) * 4, g[j]);
      }
      if (c[j] < best.c) best.c = c[j], best.index = r[j], best_cell = cell[j];  // (a lane's rows come in increasing order)
    }
  }
  // write_path_minimum (mrs_tg_pathwave.hpp), written out: through the function this kernel's time left the parent's spread
  if (!min_clearance && !argmin) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(best.c, o);
    const int orow = __shfl_xor(best.index, o), ocell = __shfl_xor(best_cell, o);
    if (fldq::better(oc, orow, best.c, best.index)) best.c = oc, best.index = orow, best_cell = ocell;
  }
  if (lane == 0) s_c[wave] = best.c, s_row[wave] = best.index, s_cell[wave] = best_cell;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kFldWaves; ++w)
      if (fldq::better(s_c[w], s_row[w], best.c, best.index)) best.c = s_c[w], best.index = s_row[w], best_cell = s_cell[w];
    if (min_clearance) min_clearance[p] = best.c;
    if (argmin) argmin[2 * (size_t)p] = best.index, argmin[2 * (size_t)p + 1] = best_cell;
  }
}

__global__ __launch_bounds__(kFldThreads) void field_clearance_vjp_kernel(const double* __restrict__ samples,
                                                                          const int32_t* __restrict__ n_samples, int capacity,
                                                                          const double* __restrict__ fields, fldq::Geometry G,
                                                                          const int32_t* __restrict__ path_field,
                                                                          const int32_t* __restrict__ status,
                                                                          const int32_t* __restrict__ cell,
                                                                          const double* __restrict__ grad_clearance,
                                                                          double* __restrict__ grad_samples) {
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  const int f = fldq::grid_of_path(path_field, p, G.n_fields);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  for (int r = threadIdx.x; r < capacity; r += kFldThreads) {
    double gi[3] = {0.0, 0.0, 0.0};
    if (r < n) {
      double cur[3];
      load_xyz(rows, r, n, cur);
      fldq::row_gradient(cur, fields, G, f, cell[row0 + r], grad_clearance[row0 + r], gi);
    }
    store_xyz0(grad_samples + (row0 + r) * 4, gi);  // (rows from n on and a dead path's rows: zeros)
  }
}

hipError_t launch_field_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity, const double* fields,
                                  const fldq::Geometry& geometry, const int32_t* path_field, const int32_t* status,
                                  double outside_value, double* clearance, int32_t* cell, double* gradient, double* min_clearance,
                                  int32_t* argmin, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(field_clearance_kernel, dim3((unsigned)n_paths), dim3(kFldThreads), 0, stream, samples, n_samples, capacity,
                      fields, geometry, path_field, status, outside_value, clearance, cell, gradient, min_clearance, argmin);
  return hipGetLastError();
}

hipError_t launch_field_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                      const double* fields, const fldq::Geometry& geometry, const int32_t* path_field,
                                      const int32_t* status, const int32_t* cell, const double* grad_clearance,
                                      double* grad_samples, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(field_clearance_vjp_kernel, dim3((unsigned)n_paths), dim3(kFldThreads), 0, stream, samples, n_samples,
                      capacity, fields, geometry, path_field, status, cell, grad_clearance, grad_samples);
  return hipGetLastError();
}

}  // namespace mrs_tg

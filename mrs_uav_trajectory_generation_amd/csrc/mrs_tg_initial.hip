// mrs_tg_initial.hip -- the first and the last stage of optimize() as plan steps (mrs_tg_initial.hpp):
// where the trajectory starts (mrs_tg_plan_initial_condition), the edit that puts that state in front of the requested waypoints
// (mrs_tg_plan_prepend_initial_condition), the pre-trajectory of a path stamped in the future (mrs_tg_plan_splice_prediction),
// and their backward passes.  The requested waypoints are addressed by explicit vertex offsets: a path may have no vertex or one.
//   initial_condition_kernel      ONE LANE PER PATH: initq::decide, then the 16 doubles of the state block, every one a copy but
//                                 z + takeoff_height; zeros where nothing is prepended.
//   prepend_count_kernel          one lane per path: initq::prepend_plan's count to offsets[p + 1]; vertex_offsets_kernel
//                                 (mrs_tg_pathedit.hip) turns the counts into offsets.
//   prepend_write_kernel          one lane per output vertex (the launch covers n_vertices + n_paths; lanes at or behind
//                                 offsets[n_paths] leave): its path by binary search, row 0 of the state block or a requested row.
//   splice_prediction_kernel      ONE WAVEFRONT PER PATH, one lane one row of a chunk of 64.  In place the chunks go from the last
//                                 to the first, each loading all its rows before it stores any, the prefix behind the lowest one.
//   splice_prediction_vjp_kernel, initial_condition_vjp_kernel (one wavefront per path) and prepend_vjp_kernel (one lane per
//                                 requested vertex, then one per path): copies of upstream rows and zeros, nothing else.
// No LDS, no atomics, no workspace; no workgroup waits for another.  Every output element a step owns is written exactly once.
#include <hip/hip_runtime.h>

#include "../../include/mrs_tg.h"
#include "mrs_tg_device.hpp"
#include "mrs_tg_initial.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

static_assert(initq::kPrepend == MRS_TG_IC_PREPEND && initq::kFromFuture == MRS_TG_IC_FROM_FUTURE &&
                  initq::kDropFirst == MRS_TG_IC_DROP_FIRST && initq::kFromTracker == MRS_TG_IC_FROM_TRACKER &&
                  initq::kFromUav == MRS_TG_IC_FROM_UAV && initq::kFromPrediction == MRS_TG_IC_FROM_PREDICTION &&
                  initq::kInvalid == MRS_TG_IC_INVALID,
              "the decision word of the header is the ABI's");
static_assert(initq::kSpliceChunk == 64, "one lane per row of a chunk");

namespace {

constexpr int kLaneThreads = 256;

__device__ __forceinline__ void load_row(const double* row, row_pair& lo, row_pair& hi) {
  const row_pair* r = reinterpret_cast<const row_pair*>(row);
  lo = r[0], hi = r[1];
}
__device__ __forceinline__ void store_row(double* row, const row_pair& lo, const row_pair& hi) {
  row_pair* o = reinterpret_cast<row_pair*>(row);
  o[0] = lo;
  o[1] = hi;
}
__device__ __forceinline__ void store_zero_row(double* row) {
  row_pair z;
  z.x = 0.0, z.y = 0.0;
  store_row(row, z, z);
}

// the vertices a path requests, from offsets the caller built (never negative here, whatever they hold)
__device__ __forceinline__ int requested_vertices(const int32_t* __restrict__ vo, int p) {
  const int nv = vo[p + 1] - vo[p];
  return nv < 0 ? 0 : nv;
}

// what the splice and its backward pass decide for path p, from the same inputs
__device__ __forceinline__ initq::SplicePlan splice_plan_of(int p, const int32_t* n_samples, int capacity, const int32_t* status,
                                                           const int32_t* __restrict__ decision,
                                                           const int32_t* __restrict__ sample_offset,
                                                           const double* __restrict__ prediction_age,
                                                           const int32_t* __restrict__ n_pred, int pred_capacity) {
  int np = n_pred[p];
  np = np < 0 ? 0 : (np > pred_capacity ? pred_capacity : np);
  return initq::splice_plan(path_live(status, p), n_samples[p], capacity, decision[p], sample_offset[p], prediction_age[p], np);
}

}  // namespace

__global__ __launch_bounds__(kLaneThreads) void initial_condition_kernel(
    int n_paths, const int32_t* __restrict__ flags, const double* __restrict__ tracker, const double* __restrict__ tracker_age,
    const double* __restrict__ uav_pose, double takeoff_height, const double* __restrict__ path_time_offset,
    const int32_t* __restrict__ vertex_offsets, const double* __restrict__ pred_position, const double* __restrict__ pred_velocity,
    const double* __restrict__ pred_acceleration, const double* __restrict__ pred_jerk, const int32_t* __restrict__ n_pred,
    int pred_capacity, int32_t* __restrict__ decision_out, int32_t* __restrict__ sample_offset_out, double* __restrict__ initial_out) {
  const int p = blockIdx.x * kLaneThreads + threadIdx.x;
  if (p >= n_paths) return;
  const int32_t f = flags[p];
  const initq::Decision d =
      initq::decide((f & initq::kHaveTracker) != 0, tracker_age[p], (f & initq::kHaveUav) != 0, (f & initq::kDontPrepend) != 0,
                    path_time_offset[p], requested_vertices(vertex_offsets, p), n_pred[p], pred_capacity);
  decision_out[p] = d.word;
  sample_offset_out[p] = d.k;
  double* out = initial_out + (size_t)p * 16;
  row_pair lo, hi;
  if (d.word & initq::kFromPrediction) {  // (d.k <= n_pred - 1 < pred_capacity, and d.k >= 1: an offset above 0.2 s)
    const size_t row = ((size_t)p * (size_t)pred_capacity + (size_t)d.k) * 4;
    const double* const from[4] = {pred_position, pred_velocity, pred_acceleration, pred_jerk};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      load_row(from[r] + row, lo, hi);
      store_row(out + r * 4, lo, hi);
    }
  } else if (d.word & initq::kFromTracker) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      load_row(tracker + (size_t)p * 16 + r * 4, lo, hi);
      store_row(out + r * 4, lo, hi);
    }
  } else if (d.word & initq::kFromUav) {
    load_row(uav_pose + (size_t)p * 4, lo, hi);
    hi.x = accumulate(hi.x, takeoff_height);
    store_row(out, lo, hi);
#pragma unroll
    for (int r = 1; r < 4; ++r) store_zero_row(out + r * 4);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) store_zero_row(out + r * 4);
  }
}

// grad_tracker [P][4][4], grad_uav [P][4] and the rows of the four prediction arrays: one wavefront per path
__global__ __launch_bounds__(64) void initial_condition_vjp_kernel(const int32_t* __restrict__ decision,
                                                                   const int32_t* __restrict__ sample_offset,
                                                                   const double* __restrict__ grad_initial, int pred_capacity,
                                                                   double* __restrict__ grad_tracker, double* __restrict__ grad_uav,
                                                                   double* __restrict__ gp0, double* __restrict__ gp1,
                                                                   double* __restrict__ gp2, double* __restrict__ gp3) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const int32_t word = decision[p];
  const double* g = grad_initial + (size_t)p * 16;
  row_pair lo, hi;
  if (lane < 4) {
    if (word & initq::kFromTracker) {
      load_row(g + lane * 4, lo, hi);
      store_row(grad_tracker + (size_t)p * 16 + lane * 4, lo, hi);
    } else {
      store_zero_row(grad_tracker + (size_t)p * 16 + lane * 4);
    }
  } else if (lane == 4) {
    if (word & initq::kFromUav) {
      load_row(g, lo, hi);
      store_row(grad_uav + (size_t)p * 4, lo, hi);
    } else {
      store_zero_row(grad_uav + (size_t)p * 4);
    }
  }
  const int at = initq::prediction_row(word, sample_offset[p], pred_capacity);
  double* const to[4] = {gp0, gp1, gp2, gp3};
  for (int r = lane; r < pred_capacity; r += 64) {
    const size_t row = ((size_t)p * (size_t)pred_capacity + (size_t)r) * 4;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (r == at) {
        load_row(g + a * 4, lo, hi);
        store_row(to[a] + row, lo, hi);
      } else {
        store_zero_row(to[a] + row);
      }
    }
  }
}

__global__ __launch_bounds__(kLaneThreads) void prepend_count_kernel(int n_paths, const int32_t* __restrict__ vertex_offsets,
                                                                     const int32_t* __restrict__ decision,
                                                                     int32_t* __restrict__ offsets) {
  const int p = blockIdx.x * kLaneThreads + threadIdx.x;
  if (p >= n_paths) return;
  offsets[p + 1] = initq::prepend_plan(decision[p], requested_vertices(vertex_offsets, p)).count;
}

__global__ __launch_bounds__(kLaneThreads) void prepend_write_kernel(
    int n_paths, int n_vertices, const int32_t* __restrict__ vertex_offsets, const double* __restrict__ waypoints,
    const uint8_t* __restrict__ stop_at, const int32_t* __restrict__ decision, const double* __restrict__ initial,
    const int32_t* __restrict__ offsets, double* __restrict__ waypoints_out, uint8_t* __restrict__ stop_out,
    int32_t* __restrict__ source_out) {
  const long long at = (long long)blockIdx.x * kLaneThreads + threadIdx.x;
  if (at >= (long long)n_vertices + n_paths) return;
  const int o = (int)at;
  if (o >= offsets[n_paths]) return;
  const int p = last_not_above(offsets, n_paths, o);
  const int j = o - offsets[p];
  const initq::Prepend e = initq::prepend_plan(decision[p], requested_vertices(vertex_offsets, p));
  row_pair lo, hi;
  if (e.prepend && j == 0) {
    load_row(initial + (size_t)p * 16, lo, hi);
    store_row(waypoints_out + (size_t)o * 4, lo, hi);
    if (stop_out) stop_out[o] = 0;
    if (source_out) source_out[o] = -1;
    return;
  }
  const int v = vertex_offsets[p] + j - e.prepend + e.drop;
  if (v < 0 || v >= n_vertices) return;  // (offsets that do not describe the batch: nothing is read or written outside it)
  load_row(waypoints + (size_t)v * 4, lo, hi);
  store_row(waypoints_out + (size_t)o * 4, lo, hi);
  if (stop_out) stop_out[o] = stop_at ? stop_at[v] : (uint8_t)0;
  if (source_out) source_out[o] = v;
}

// lanes 0 .. n_vertices-1: the requested vertices; lanes n_vertices .. n_vertices + n_paths - 1: row 0 of a path's state block
__global__ __launch_bounds__(kLaneThreads) void prepend_vjp_kernel(int n_paths, int n_vertices,
                                                                   const int32_t* __restrict__ vertex_offsets,
                                                                   const int32_t* __restrict__ decision,
                                                                   const int32_t* __restrict__ offsets, int n_edited,
                                                                   const double* __restrict__ grad_edited,
                                                                   double* __restrict__ grad_waypoints,
                                                                   double* __restrict__ grad_initial_row) {
  const long long at = (long long)blockIdx.x * kLaneThreads + threadIdx.x;
  if (at >= (long long)n_vertices + n_paths) return;
  row_pair lo, hi;
  if (at >= n_vertices) {
    const int p = (int)(at - n_vertices);
    const initq::Prepend e = initq::prepend_plan(decision[p], requested_vertices(vertex_offsets, p));
    const int o = offsets[p];
    if (e.prepend && o >= 0 && o < n_edited) {
      load_row(grad_edited + (size_t)o * 4, lo, hi);
      store_row(grad_initial_row + (size_t)p * 4, lo, hi);
    } else {
      store_zero_row(grad_initial_row + (size_t)p * 4);
    }
    return;
  }
  const int v = (int)at;
  const int p = last_not_above(vertex_offsets, n_paths, v);
  const int i = v - vertex_offsets[p];
  const initq::Prepend e = initq::prepend_plan(decision[p], requested_vertices(vertex_offsets, p));
  const int o = offsets[p] + i - e.drop + e.prepend;
  if (i < e.drop || o < 0 || o >= n_edited || o >= offsets[p + 1]) {  // the dropped vertex
    store_zero_row(grad_waypoints + (size_t)v * 4);
    return;
  }
  load_row(grad_edited + (size_t)o * 4, lo, hi);
  store_row(grad_waypoints + (size_t)v * 4, lo, hi);
}

// (samples_out may be samples, n_samples_out may be n_samples, status_out may be status)
__global__ __launch_bounds__(64) void splice_prediction_kernel(const double* samples, const int32_t* n_samples, int capacity,
                                                               const int32_t* status, const int32_t* __restrict__ decision,
                                                               const int32_t* __restrict__ sample_offset,
                                                               const double* __restrict__ prediction_age,
                                                               const double* __restrict__ pred_position,
                                                               const int32_t* __restrict__ n_pred, int pred_capacity,
                                                               double* samples_out, int32_t* n_samples_out, int32_t* status_out) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const bool live = path_live(status, p);
  const int n_in = n_samples[p];
  const int st_in = status ? status[p] : (int)MRS_TG_STATUS_SUCCESS;
  const initq::SplicePlan s = splice_plan_of(p, n_samples, capacity, status, decision, sample_offset, prediction_age, n_pred,
                                             pred_capacity);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* rows = samples + row0 * 4;
  double* out = samples_out + row0 * 4;
  const bool in_place = samples_out == samples;
  row_pair lo, hi;
  if (s.action != initq::kInsert) {
    if (!in_place && live) {  // the rows pass through
      const int n = live_samples(true, n_samples, p, capacity);
      for (int i = lane; i < n; i += 64) {
        load_row(rows + (size_t)i * 4, lo, hi);
        store_row(out + (size_t)i * 4, lo, hi);
      }
    }
    if (lane == 0) {
      n_samples_out[p] = s.action == initq::kTooLong ? s.count : n_in;
      if (status_out) status_out[p] = s.action == initq::kShort ? (int)MRS_TG_STATUS_INVALID_ARGS : st_in;
    }
    return;
  }
  const int n = s.n, k = s.k;  // n + k <= capacity, k <= n_pred <= pred_capacity
  for (int c = initq::splice_chunks(n) - 1; c >= 0; --c) {
    const int i = c * initq::kSpliceChunk + lane;
    if (i < n) load_row(rows + (size_t)i * 4, lo, hi);
    __builtin_amdgcn_wave_barrier();  // every row of the chunk is loaded before one is stored
    if (i < n) store_row(out + (size_t)(i + k) * 4, lo, hi);
  }
  const double* pre = pred_position + (size_t)p * (size_t)pred_capacity * 4;
  for (int i = lane; i < k; i += 64) {
    load_row(pre + (size_t)i * 4, lo, hi);
    store_row(out + (size_t)i * 4, lo, hi);
  }
  if (lane == 0) {
    n_samples_out[p] = s.count;
    if (status_out) status_out[p] = st_in;
  }
}

__global__ __launch_bounds__(64) void splice_prediction_vjp_kernel(const int32_t* __restrict__ n_samples, int capacity,
                                                                   const int32_t* __restrict__ status,
                                                                   const int32_t* __restrict__ decision,
                                                                   const int32_t* __restrict__ sample_offset,
                                                                   const double* __restrict__ prediction_age,
                                                                   const int32_t* __restrict__ n_pred, int pred_capacity,
                                                                   const double* __restrict__ grad_out,
                                                                   double* __restrict__ grad_samples,
                                                                   double* __restrict__ grad_pred_position) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const initq::SplicePlan s = splice_plan_of(p, n_samples, capacity, status, decision, sample_offset, prediction_age, n_pred,
                                             pred_capacity);
  const bool insert = s.action == initq::kInsert;
  const int n = insert ? s.n : live_samples(path_live(status, p), n_samples, p, capacity);
  const int k = insert ? s.k : 0;
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* up = grad_out + row0 * 4;
  double* gs = grad_samples + row0 * 4;
  double* gp = grad_pred_position + (size_t)p * (size_t)pred_capacity * 4;
  row_pair lo, hi;
  for (int i = lane; i < capacity; i += 64) {
    if (i < n) {
      load_row(up + (size_t)(i + k) * 4, lo, hi);
      store_row(gs + (size_t)i * 4, lo, hi);
    } else {
      store_zero_row(gs + (size_t)i * 4);
    }
  }
  for (int i = lane; i < pred_capacity; i += 64) {
    if (i < k) {
      load_row(up + (size_t)i * 4, lo, hi);
      store_row(gp + (size_t)i * 4, lo, hi);
    } else {
      store_zero_row(gp + (size_t)i * 4);
    }
  }
}

hipError_t launch_initial_condition(int n_paths, const int32_t* flags, const double* tracker, const double* tracker_age,
                                    const double* uav_pose, double takeoff_height, const double* path_time_offset,
                                    const int32_t* vertex_offsets, const double* const pred[4], const int32_t* n_pred,
                                    int pred_capacity, int32_t* decision_out, int32_t* sample_offset_out, double* initial_out,
                                    hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(initial_condition_kernel, dim3(cdiv(n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream, n_paths, flags,
                      tracker, tracker_age, uav_pose, takeoff_height, path_time_offset, vertex_offsets, pred[0], pred[1], pred[2],
                      pred[3], n_pred, pred_capacity, decision_out, sample_offset_out, initial_out);
  return hipGetLastError();
}

hipError_t launch_initial_condition_vjp(int n_paths, const int32_t* decision, const int32_t* sample_offset,
                                        const double* grad_initial, int pred_capacity, double* grad_tracker, double* grad_uav,
                                        double* const grad_pred[4], hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(initial_condition_vjp_kernel, dim3((unsigned)n_paths), dim3(64), 0, stream, decision, sample_offset,
                      grad_initial, pred_capacity, grad_tracker, grad_uav, grad_pred[0], grad_pred[1], grad_pred[2], grad_pred[3]);
  return hipGetLastError();
}

hipError_t launch_prepend_initial_condition(int n_paths, int n_vertices, const int32_t* vertex_offsets, const double* waypoints,
                                            const uint8_t* stop_at, const int32_t* decision, const double* initial,
                                            int32_t* offsets, double* waypoints_out, uint8_t* stop_out, int32_t* source_out,
                                            hipStream_t stream) {
  const KernelTimer kt = take_kernel_timer();
  if (n_paths > 0) {
    MRS_TG_LAUNCH_EXT(prepend_count_kernel, dim3(cdiv(n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream, kt.start, nullptr, 0,
                      n_paths, vertex_offsets, decision, offsets);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  const bool rows = n_paths > 0;
  if (hipError_t e = launch_vertex_offsets(n_paths, offsets, n_paths > 0 ? nullptr : kt.start, rows ? nullptr : kt.stop, stream);
      e != hipSuccess)
    return e;
  if (!rows) return hipSuccess;
  MRS_TG_LAUNCH_EXT(prepend_write_kernel, dim3(cdiv((long long)n_vertices + n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream,
                    nullptr, kt.stop, 0, n_paths, n_vertices, vertex_offsets, waypoints, stop_at, decision, initial, offsets,
                    waypoints_out, stop_out, source_out);
  return hipGetLastError();
}

hipError_t launch_prepend_initial_condition_vjp(int n_paths, int n_vertices, const int32_t* vertex_offsets, const int32_t* decision,
                                                const int32_t* offsets, int n_edited, const double* grad_edited,
                                                double* grad_waypoints, double* grad_initial_row, hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(prepend_vjp_kernel, dim3(cdiv((long long)n_vertices + n_paths, kLaneThreads)), dim3(kLaneThreads), 0, stream,
                      n_paths, n_vertices, vertex_offsets, decision, offsets, n_edited, grad_edited, grad_waypoints,
                      grad_initial_row);
  return hipGetLastError();
}

hipError_t launch_splice_prediction(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                    const int32_t* status, const int32_t* decision, const int32_t* sample_offset,
                                    const double* prediction_age, const double* pred_position, const int32_t* n_pred,
                                    int pred_capacity, double* samples_out, int32_t* n_samples_out, int32_t* status_out,
                                    hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(splice_prediction_kernel, dim3((unsigned)n_paths), dim3(64), 0, stream, samples, n_samples, capacity, status,
                      decision, sample_offset, prediction_age, pred_position, n_pred, pred_capacity, samples_out, n_samples_out,
                      status_out);
  return hipGetLastError();
}

hipError_t launch_splice_prediction_vjp(int n_paths, const int32_t* n_samples, int capacity, const int32_t* status,
                                        const int32_t* decision, const int32_t* sample_offset, const double* prediction_age,
                                        const int32_t* n_pred, int pred_capacity, const double* grad_out, double* grad_samples,
                                        double* grad_pred_position, hipStream_t stream) {
  if (n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(splice_prediction_vjp_kernel, dim3((unsigned)n_paths), dim3(64), 0, stream, n_samples, capacity, status,
                      decision, sample_offset, prediction_age, n_pred, pred_capacity, grad_out, grad_samples, grad_pred_position);
  return hipGetLastError();
}

}  // namespace mrs_tg

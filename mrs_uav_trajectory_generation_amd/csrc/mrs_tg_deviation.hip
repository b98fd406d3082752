// mrs_tg_deviation.hip -- how far the sampled trajectory strays from the waypoint polyline (mrs_tg_plan_path_deviation) and
// its backward pass (mrs_tg_plan_path_deviation_vjp); mrs_tg_deviation.hpp, DESIGN.md section 11b.  The scan is
// validateTrajectorySpatial's: a waypoint cursor that moves on when the step to the next sample passes the next waypoint.
// ONE WAVEFRONT TAKES ONE PATH, ONE LANE ONE SAMPLE of a chunk of 64.  The cursor is the only serial part; a chunk resolves
// it by ballots (resolve_cursors): all open lanes test the advance against the same waypoint, the first lane that advances
// closes the lanes up to itself, the cursor moves on, the lanes behind test again -- advances + 1 rounds per chunk.
//   path_deviation_kernel      the deviation of every sample is then one evaluation per lane; the maxima are wavefront
//                              reductions, the first index winning on equal values.
//   path_deviation_vjp_kernel  resolves the same cursors, forms a sample's three gradient rows in its lane, stores the sample's
//                              own and parks the two waypoint rows in an LDS tile [64][6]; six lanes then add them up, one
//                              sample per step in increasing index, an accumulator moving on with the cursor.
// A chunk's global loads -- its samples, the next chunk's (whose first is lane 63's neighbour: the seam), the upstream -- are
// issued in one round in front of the rounds' arithmetic and of the chunk's stores (rule 1: on gfx950
// loads and stores retire through one counter).  Reads only; no atomics, no workspace; every output element written once.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_deviation.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

namespace {

constexpr int kDevTileStride = 7;  // doubles between the parked rows [6] of two samples (odd: no bank is hit twice by a row)

// The cursors of a chunk.  c: the cursor at the chunk's first sample, wavefront-uniform; on return the cursor at the next
// chunk's first sample.  scanned: whether the lane holds a sample of the scan (i < n - 1).  Returns the lane's cursor (-1
// for a lane that is not scanned).
__device__ __forceinline__ int resolve_cursors(const double* s_w, const double (&s)[3], const double (&nx)[3], bool scanned,
                                               int lane, int S, int& c) {
  int mine = -1;
  bool open = scanned;
  for (;;) {
    const double wb[3] = {s_w[3 * (c + 1)], s_w[3 * (c + 1) + 1], s_w[3 * (c + 1) + 2]};
    const bool adv = open && devq::advances(wb, s, nx, c, S);
    const unsigned long long m = __ballot(adv);
    if (m == 0) {
      if (open) mine = c;
      break;
    }
    const int f = __ffsll((long long)m) - 1;
    if (open && lane <= f) {
      mine = c;
      open = false;
    }
    ++c;
    if (__ballot(open) == 0) break;
  }
  return mine;
}

}  // namespace

__global__ __launch_bounds__(64) void path_deviation_kernel(BatchView b, const double* __restrict__ samples,
                                                            const int32_t* __restrict__ n_samples,
                                                            const double* __restrict__ waypoints, int capacity,
                                                            int first_segment, const int32_t* __restrict__ status,
                                                            double* __restrict__ deviation, int32_t* __restrict__ cursor,
                                                            double* __restrict__ max_deviation, int32_t* __restrict__ argmax,
                                                            double* __restrict__ segment_max) {
  // [max_segments + 1][3] waypoints | [max_segments] segment maxima
  extern __shared__ double s_w[];
  double* s_m = s_w + 3 * (b.max_segments + 1);
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  const int n = live_samples(path_live(status, pr.p), n_samples, pr.p, capacity);
  for (int e = lane; e < 3 * (S + 1); e += 64) s_w[e] = waypoints[(size_t)(pr.v0 + e / 3) * 4 + e % 3];
  for (int i = lane; i < S; i += 64) s_m[i] = 0.0;
  const size_t row0 = (size_t)pr.p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  double cur[3];
  load_xyz(rows, lane, n, cur);
  wave_lds_barrier();
  int c = 0, run_arg = -1;
  double run_max = 0.0;
  for (int k0 = 0; k0 < n - 1; k0 += 64) {
    const int i = k0 + lane;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    seam_neighbour(cur, nxt, lane, nx);
    const bool scanned = i < n - 1;
    const int c_first = c;
    const int mine = resolve_cursors(s_w, cur, nx, scanned, lane, S, c);
    double d = 0.0;
    if (scanned) d = devq::dist(cur, s_w + 3 * mine, s_w + 3 * mine + 3);
    const bool cnt = scanned && devq::counted(mine, first_segment, S);
    if (max_deviation || argmax) {
      const double cm = wave_max(cnt ? d : 0.0);
      if (cm > run_max) {  // (strictly: the running maximum of the reference keeps the first sample that reaches a value)
        run_max = cm;
        run_arg = k0 + __ffsll((long long)__ballot(cnt && d == cm)) - 1;
      }
    }
    if (segment_max) {
      for (int cv = c_first; cv <= c && cv < S; ++cv) {
        const double m = wave_max(cnt && mine == cv ? d : 0.0);
        if (lane == 0) s_m[cv] = fmax(s_m[cv], m);
      }
    }
    if (scanned) {
      if (deviation) deviation[row0 + i] = d;
      if (cursor) cursor[row0 + i] = mine;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  for (int i = (n > 1 ? n - 1 : 0) + lane; i < capacity; i += 64) {
    if (deviation) deviation[row0 + i] = 0.0;
    if (cursor) cursor[row0 + i] = -1;
  }
  if (lane == 0) {
    if (max_deviation) max_deviation[pr.p] = run_max;
    if (argmax) argmax[pr.p] = run_arg;
  }
  if (segment_max) {
    wave_lds_barrier();
    for (int i = lane; i < S; i += 64) segment_max[pr.s0 + i] = s_m[i];
  }
}

__global__ __launch_bounds__(64) void path_deviation_vjp_kernel(BatchView b, const double* __restrict__ samples,
                                                                const int32_t* __restrict__ n_samples,
                                                                const double* __restrict__ waypoints, int capacity,
                                                                const int32_t* __restrict__ status,
                                                                const double* __restrict__ grad_deviation,
                                                                double* __restrict__ grad_samples,
                                                                double* __restrict__ grad_waypoints) {
  // [max_segments + 1][3] waypoints | [max_segments + 1][3] their gradients | [64][7] tile | [64] cursors of the parked samples
  extern __shared__ double s_w[];
  double* s_gw = s_w + 3 * (b.max_segments + 1);
  double* s_tile = s_gw + 3 * (b.max_segments + 1);
  int* s_cur = reinterpret_cast<int*>(s_tile + 64 * kDevTileStride);
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  // live_samples of mrs_tg_pathwave.hpp, written out: through the function this kernel gets another register allocation
  const bool live = path_live(status, pr.p);
  int n = live ? min(n_samples[pr.p], capacity) : 0;
  n = n < 0 ? 0 : n;
  for (int e = lane; e < 3 * (S + 1); e += 64) {
    s_w[e] = waypoints[(size_t)(pr.v0 + e / 3) * 4 + e % 3];
    s_gw[e] = 0.0;
  }
  const size_t row0 = (size_t)pr.p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  double cur[3];
  load_xyz(rows, lane, n, cur);
  wave_lds_barrier();
  const int slot = min(lane, 5);  // lanes 0..2: the waypoint at the cursor, 3..5: the one behind it (the others follow lane 5 and store nothing)
  const bool owns = lane < 6;
  int c = 0, acc_c = 0;  // acc_c: the cursor the accumulators belong to
  double acc = 0.0;
  for (int k0 = 0; k0 < n - 1; k0 += 64) {
    const int i = k0 + lane;
    const bool scanned = i < n - 1;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    const double g = scanned ? grad_deviation[row0 + i] : 0.0;
    seam_neighbour(cur, nxt, lane, nx);
    const int mine = resolve_cursors(s_w, cur, nx, scanned, lane, S, c);
    double gp[3] = {0.0, 0.0, 0.0}, ga[3] = {0.0, 0.0, 0.0}, gb[3] = {0.0, 0.0, 0.0};
    if (scanned) devq::dist_vjp(cur, s_w + 3 * mine, s_w + 3 * mine + 3, g, gp, ga, gb);
    if (grad_samples && scanned) store_xyz0(grad_samples + (row0 + i) * 4, gp);
    if (grad_waypoints) {
      double* row = s_tile + lane * kDevTileStride;
#pragma unroll
      for (int k = 0; k < 3; ++k) row[k] = ga[k], row[3 + k] = gb[k];
      s_cur[lane] = mine;
      wave_lds_barrier();
      const int count = min(64, n - 1 - k0);
      for (int r = 0; r < count; ++r) {
        const int cr = __builtin_amdgcn_readfirstlane(s_cur[r]);
        while (acc_c < cr) {  // the cursor moved on: the waypoint at it is complete, the one behind it becomes the one at it
          if (lane < 3) s_gw[3 * acc_c + lane] = acc;
          const double behind = __shfl(acc, (lane + 3) & 63);
          acc = lane < 3 ? behind : 0.0;
          ++acc_c;
        }
        acc = devq::accumulate(acc, s_tile[r * kDevTileStride + slot]);
      }
      wave_lds_barrier();  // (the next chunk overwrites the tile)
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  if (grad_samples) {
    row_pair zero;
    zero.x = 0.0, zero.y = 0.0;
    row_pair* out = reinterpret_cast<row_pair*>(grad_samples + row0 * 4);
    for (int e = 2 * (n > 1 ? n - 1 : 0) + lane; e < 2 * capacity; e += 64) out[e] = zero;
  }
  if (grad_waypoints) {
    if (owns) s_gw[3 * acc_c + lane] = acc;
    wave_lds_barrier();
    for (int e = lane; e < 4 * (S + 1); e += 64)
      grad_waypoints[(size_t)pr.v0 * 4 + e] = e % 4 < 3 ? s_gw[3 * (e / 4) + e % 4] : 0.0;
  }
}

hipError_t launch_path_deviation(const BatchView& b, const double* samples, const int32_t* n_samples, const double* waypoints,
                                 int capacity, int first_segment, const int32_t* status, double* deviation, int32_t* cursor,
                                 double* max_deviation, int32_t* argmax, double* segment_max, hipStream_t stream) {
  const size_t lds = sizeof(double) * (3 * ((size_t)b.max_segments + 1) + (size_t)b.max_segments);
  if (b.n_paths == 0) return empty_batch_lds(lds);
  const auto fwd = MRS_TG_KERNEL(path_deviation_kernel);
  if (hipError_t e = prepare_dynamic_lds(fwd, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(fwd, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, samples, n_samples, waypoints, capacity,
                      first_segment, status, deviation, cursor, max_deviation, argmax, segment_max);
  return hipGetLastError();
}

hipError_t launch_path_deviation_vjp(const BatchView& b, const double* samples, const int32_t* n_samples,
                                     const double* waypoints, int capacity, const int32_t* status, const double* grad_deviation,
                                     double* grad_samples, double* grad_waypoints, hipStream_t stream) {
  const size_t lds = sizeof(double) * (6 * ((size_t)b.max_segments + 1) + 64 * kDevTileStride) + sizeof(int) * 64;
  if (b.n_paths == 0) return empty_batch_lds(lds);
  const auto vjp = MRS_TG_KERNEL(path_deviation_vjp_kernel);
  if (hipError_t e = prepare_dynamic_lds(vjp, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(vjp, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, samples, n_samples, waypoints, capacity, status,
                      grad_deviation, grad_samples, grad_waypoints);
  return hipGetLastError();
}

}  // namespace mrs_tg

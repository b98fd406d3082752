// mrs_tg_fallback.hip -- the fallback sampler as a plan step (mrs_tg_plan_fallback_sample), its backward pass
// (mrs_tg_plan_fallback_sample_vjp) and the heading unwrap (mrs_tg_plan_unwrap_headings); mrs_tg_fallback.hpp, DESIGN.md
// section 11d.
//   unwrap_headings_kernel      one lane per path, the scan over its vertices serial (vertex v against the unwrapped v - 1).
//   fallback_sample_kernel      ONE WAVEFRONT TAKES ONE PATH.  Phase A (count_rows): lane = segment in chunks of 64, the row rule,
//                               an inclusive wavefront prefix less the lane's own rows, a carry across chunks (64-bit sums); first
//                               row, divisor and dwell of every segment stay in LDS beside the path's waypoints.  Phase B: lane
//                               = output row in chunks of 64, its segment by binary search over the first rows in LDS, the row
//                               formed in the lane and stored as 32 bytes: a wave instruction writes 2 KB without gaps.
//   fallback_sample_vjp_kernel  the same phase A, so the forward's counts; a chunk's 64 upstream rows loaded as a wavefront and
//                               parked in an LDS tile with each row's segment and coefficient; eight lanes then add them up in
//                               row order, four towards the segment's first vertex and four towards its second, the
//                               accumulators moving on with the segment (as path_deviation_vjp_kernel sums its waypoint rows).
// LDS is sized by the plan's longest path (16 bytes a segment for phase A, the forward's waypoint copy 32 bytes a vertex, the
// backward pass's tile 2.6 KB): 0.5 KB and 2.9 KB at ten segments, 12.3 KB and 6.9 KB at MRS_TG_MAX_SEGMENTS, so the short paths
// of a large batch are not held to the occupancy of the longest path a plan can hold.  Reads only; no atomics, no workspace;
// n_samples, seg_first_row and grad_waypoints are written exactly once per element, the sample rows below min(count, capacity)
// exactly once and the rows from there on not at all.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_fallback.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

namespace {

constexpr int kUnwrapThreads = 64;
constexpr int kFbTileStride = 5;  // doubles between the parked rows of two samples: g [4] and the coefficient (odd)

// what phase A leaves in LDS for a path, [max_segments] each
struct PathRows {
  double* nd;   // the divisor of a segment's step
  int* first;   // the row its samples start at, saturated at capacity + 1
  int* dwell;   // rows inserted behind its first
};
// the arrays inside the kernel's dynamic LDS: the doubles in front (nd, then `doubles_between` of the kernel's own), the ints behind
__device__ __forceinline__ PathRows path_rows(double* lds, int max_segments, int doubles_between) {
  PathRows s;
  s.nd = lds;
  s.first = reinterpret_cast<int*>(lds + max_segments + doubles_between);
  s.dwell = s.first + max_segments;
  return s;
}
constexpr size_t path_rows_bytes(int max_segments) { return (sizeof(double) + 2 * sizeof(int)) * (size_t)max_segments; }

__device__ __forceinline__ long long wave_inclusive_sum(long long v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

// Phase A of both kernels -> the path's row count (64-bit; wavefront-uniform)
__device__ __forceinline__ long long count_rows(const PathRows& s, const double* __restrict__ seg_times,
                                                const uint8_t* __restrict__ stop_at, int S, double dt, int insert,
                                                int capacity, int lane, int32_t* __restrict__ seg_first_row_out) {
  long long carry = 0;
  for (int i0 = 0; i0 < S; i0 += 64) {
    const int i = i0 + lane;
    fbq::SegmentRows r;
    r.nd = 0.0, r.dwell = 0, r.rows = 0;
    if (i < S) r = fbq::segment_rows(seg_times[i], dt, insert, i, S, stop_at != nullptr && stop_at[i] != 0);
    const long long incl = wave_inclusive_sum(r.rows, lane);
    if (i < S) {
      const int first = fbq::saturated(carry + incl - r.rows, capacity);
      s.first[i] = first, s.dwell[i] = r.dwell, s.nd[i] = r.nd;
      if (seg_first_row_out) seg_first_row_out[i] = first;
    }
    carry += __shfl(incl, 63);
  }
  return carry;
}

}  // namespace

__global__ __launch_bounds__(kUnwrapThreads) void unwrap_headings_kernel(BatchView b, const double* wp, double* out) {
  const int p = (int)blockIdx.x * kUnwrapThreads + (int)threadIdx.x;
  if (p >= b.n_paths) return;
  const int seg0 = first_segment(b, p);
  const int S = segments_of(b, p, seg0);
  const size_t v0 = (size_t)(seg0 + p) * 4;
  fbq::unwrap_path(wp + v0, S + 1, out + v0);  // (out may be wp: a vertex is read before it is written, and only by this lane)
}

__global__ __launch_bounds__(64) void fallback_sample_kernel(BatchView b, const double* __restrict__ waypoints,
                                                             const uint8_t* __restrict__ stop_at,
                                                             const double* __restrict__ seg_times, double dt, int insert,
                                                             int capacity, int32_t* __restrict__ n_samples,
                                                             double* __restrict__ samples, int32_t* __restrict__ seg_first_row) {
  // [max_segments] divisors | [max_segments + 1][4] waypoints | [max_segments] first rows | [max_segments] dwells
  extern __shared__ double s_lds[];
  const PathRows s = path_rows(s_lds, b.max_segments, 4 * (b.max_segments + 1));
  double* s_w = s_lds + b.max_segments;
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  for (int e = lane; e < 4 * (S + 1); e += 64) s_w[e] = waypoints[(size_t)pr.v0 * 4 + e];
  const long long count = count_rows(s, seg_times + pr.s0, stop_at ? stop_at + pr.v0 : nullptr, S, dt, insert, capacity, lane,
                                     seg_first_row ? seg_first_row + pr.s0 : nullptr);
  if (lane == 0) n_samples[pr.p] = fbq::saturated(count, capacity);
  wave_lds_barrier();
  const int n = count < (long long)capacity ? (int)count : capacity;
  double* __restrict__ rows = samples + (size_t)pr.p * (size_t)capacity * 4;
  for (int r = lane; r < n; r += 64) {
    const int i = fbq::segment_of_row(s.first, S, r);
    const double coeff = fbq::row_coeff(s.nd[i], s.dwell[i], r - s.first[i]);
    double p[4];
    fbq::row_at(s_w + 4 * i, s_w + 4 * i + 4, coeff, p);
    row_pair* out = reinterpret_cast<row_pair*>(rows + (size_t)r * 4);
    row_pair lo, hi;
    lo.x = p[0], lo.y = p[1], hi.x = p[2], hi.y = p[3];
    out[0] = lo;
    out[1] = hi;
  }
}

__global__ __launch_bounds__(64) void fallback_sample_vjp_kernel(BatchView b, const uint8_t* __restrict__ stop_at,
                                                                 const double* __restrict__ seg_times, double dt, int insert,
                                                                 int capacity, const double* __restrict__ grad_samples,
                                                                 double* __restrict__ grad_waypoints) {
  // [max_segments] divisors | [64][5] tile | [max_segments] first rows | [max_segments] dwells | [64] segments of the parked rows
  extern __shared__ double s_lds[];
  const PathRows s = path_rows(s_lds, b.max_segments, 64 * kFbTileStride);
  double* s_tile = s_lds + b.max_segments;
  int* s_seg = s.dwell + b.max_segments;
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  const long long count = count_rows(s, seg_times + pr.s0, stop_at ? stop_at + pr.v0 : nullptr, S, dt, insert, capacity, lane,
                                     nullptr);
  wave_lds_barrier();
  const int n = count < (long long)capacity ? (int)count : capacity;
  const row_pair* __restrict__ rows = reinterpret_cast<const row_pair*>(grad_samples + (size_t)pr.p * (size_t)capacity * 4);
  double* __restrict__ gw = grad_waypoints + (size_t)pr.v0 * 4;
  // lanes 0..3: the columns of the vertex the segment starts at (weight 1 - coeff), 4..7: of the one it ends at (weight coeff);
  // the other lanes follow lane 7 and store nothing
  const int col = lane & 3;
  const bool to_b = lane >= 4;
  int acc_i = 0;  // the segment the accumulators belong to
  double acc = 0.0;
  row_pair lo, hi;
  lo.x = lo.y = hi.x = hi.y = 0.0;
  if (lane < n) lo = rows[2 * (size_t)lane], hi = rows[2 * (size_t)lane + 1];
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int r = k0 + lane;
    row_pair nlo, nhi;  // the next chunk's upstream rows: issued in front of this chunk's walk
    nlo.x = nlo.y = nhi.x = nhi.y = 0.0;
    if (r + 64 < n) nlo = rows[2 * (size_t)(r + 64)], nhi = rows[2 * (size_t)(r + 64) + 1];
    int i = 0;
    double coeff = 0.0;
    if (r < n) {
      i = fbq::segment_of_row(s.first, S, r);
      coeff = fbq::row_coeff(s.nd[i], s.dwell[i], r - s.first[i]);
    }
    double* row = s_tile + lane * kFbTileStride;
    row[0] = lo.x, row[1] = lo.y, row[2] = hi.x, row[3] = hi.y, row[4] = coeff;
    s_seg[lane] = i;
    wave_lds_barrier();
    const int rows_here = min(64, n - k0);
    for (int q = 0; q < rows_here; ++q) {
      const int iq = __builtin_amdgcn_readfirstlane(s_seg[q]);
      while (acc_i < iq) {  // the segment moved on: its first vertex is complete, its second becomes the next one's first
        if (lane < 4) gw[4 * acc_i + lane] = acc;
        const double behind = __shfl(acc, (lane + 4) & 63);
        acc = lane < 4 ? behind : 0.0;
        ++acc_i;
      }
      const double c = s_tile[q * kFbTileStride + 4], g = s_tile[q * kFbTileStride + col];
      acc = fbq::accumulate(acc, to_b ? fbq::towards_b(c, g) : fbq::towards_a(c, g));
    }
    wave_lds_barrier();  // (the next chunk overwrites the tile)
    lo = nlo, hi = nhi;
  }
  if (lane < 8) gw[4 * acc_i + lane] = acc;  // vertices acc_i and acc_i + 1 (acc_i <= S - 1); the ones behind them are zero
  for (int e = 4 * (acc_i + 2) + lane; e < 4 * (S + 1); e += 64) gw[e] = 0.0;
}

hipError_t launch_unwrap_headings(const BatchView& b, const double* wp, double* out, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(unwrap_headings_kernel, dim3(cdiv(b.n_paths, kUnwrapThreads)), dim3(kUnwrapThreads), 0, stream, b, wp,
                      out);
  return hipGetLastError();
}

hipError_t launch_fallback_sample(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const double* seg_times,
                                  double dt, int insert, int capacity, int32_t* n_samples, double* samples,
                                  int32_t* seg_first_row, hipStream_t stream) {
  const size_t lds = path_rows_bytes(b.max_segments) + sizeof(double) * 4 * ((size_t)b.max_segments + 1);
  if (b.n_paths <= 0) return empty_batch_lds(lds);
  const auto fwd = MRS_TG_KERNEL(fallback_sample_kernel);
  if (hipError_t e = prepare_dynamic_lds(fwd, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(fwd, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, waypoints, stop_at, seg_times, dt, insert,
                      capacity, n_samples, samples, seg_first_row);
  return hipGetLastError();
}

hipError_t launch_fallback_sample_vjp(const BatchView& b, const uint8_t* stop_at, const double* seg_times, double dt, int insert,
                                      int capacity, const double* grad_samples, double* grad_waypoints, hipStream_t stream) {
  const size_t lds = path_rows_bytes(b.max_segments) + sizeof(double) * 64 * kFbTileStride + sizeof(int) * 64;
  if (b.n_paths <= 0) return empty_batch_lds(lds);
  const auto vjp = MRS_TG_KERNEL(fallback_sample_vjp_kernel);
  if (hipError_t e = prepare_dynamic_lds(vjp, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(vjp, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, stop_at, seg_times, dt, insert, capacity,
                      grad_samples, grad_waypoints);
  return hipGetLastError();
}

}  // namespace mrs_tg

// mrs_tg_pathedit.hip -- path thinning (mrs_tg_plan_preprocess_path), mid-point subdivision (mrs_tg_plan_insert_midpoints) and
// their one backward pass (mrs_tg_plan_path_edit_vjp); mrs_tg_pathedit.hpp, DESIGN.md section 11e.  An edit writes a PACKED
// batch with its own vertex offsets, in three launches on one stream:
//   thin_path_kernel          ONE WAVEFRONT TAKES ONE PATH.  From the last kept vertex the 64 lanes judge the candidates base +
//                             lane against it (pathq::keeps), a ballot picks the first kept one, which becomes `last`; an empty
//                             ballot moves the window on by 64 under the same `last`.  The input index of the k-th kept vertex
//                             goes to slot k of the path's own vertices in the plan's scratch, the count to offsets[p + 1].
//   insert_midpoints_kernel   ONE WAVEFRONT TAKES ONE PATH.  Lane = segment in chunks of 64: the rule (pathq::inserts), an
//                             inclusive wavefront sum of 1 + inserted with a carry across chunks; slot i of the scratch gets the
//                             place of input vertex i in the edited path, offsets[p + 1] the count.
//   vertex_offsets_kernel     ONE WORKGROUP: the counts at offsets[1 ..] become their running sum in place, offsets[0] = 0; the
//                             paths in chunks of kPathEditScanChunk, the sum carried from chunk to chunk in a register.  No workgroup
//                             of this file waits for another one: no look-back, no spin loop, no atomics.
//   edit_write_kernel         one lane per output vertex (the launch covers the upper bound sum V or sum V + sum S; lanes at or
//                             behind offsets[n_paths] leave): its path by binary search over the offsets, its input vertex from the
//                             scratch -- by index after thinning, by binary search over the places after subdivision, where a
//                             place that no input vertex has is a mid-point (pathq::interpolate_point at 0.5).
//   path_edit_vjp_kernel      one lane per INPUT vertex: pathq::edit_gradient on its path's run of source / inserted.
// No LDS beside the scan's 16 wave totals.  Every output element below offsets[n_paths] is written exactly once, nothing at or
// behind it; grad_waypoints is written exactly once per element of the plan.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathedit.hpp"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

namespace {

constexpr int kWriteThreads = 256;
static_assert(kPathEditScanChunk % 64 == 0 && kPathEditScanChunk <= 1024, "whole wavefronts of one workgroup");

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o);
    if (lane >= o) v += up;
  }
  return v;
}

}  // namespace

__global__ __launch_bounds__(64) void thin_path_kernel(BatchView b, const double* __restrict__ waypoints, pathq::ThinOptions o,
                                                       int32_t* __restrict__ kept_ws, int32_t* __restrict__ offsets) {
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int n = pr.S + 1;
  const double* __restrict__ w = waypoints + (size_t)pr.v0 * 4;
  int32_t* __restrict__ kept = kept_ws + pr.v0;
  if (lane == 0) kept[0] = 0;
  int count = 1, last = 0, base = 1;  // wavefront-uniform
  while (base < n) {
    const int c = base + lane;
    const bool keep = c < n && pathq::keeps(w, 4, n, last, c, o);
    const unsigned long long found = __ballot(keep);
    if (found == 0ull) {
      base += pathq::kWindow;
      continue;
    }
    last = base + (__ffsll(found) - 1);
    if (lane == 0) kept[count] = last;  // (count <= last < n: inside the path's own slots)
    ++count;
    base = last + 1;
  }
  if (lane == 0) offsets[pr.p + 1] = count;
}

__global__ __launch_bounds__(64) void insert_midpoints_kernel(BatchView b, const double* __restrict__ segment_max,
                                                              double max_deviation, int first_segment,
                                                              const uint8_t* __restrict__ active, int32_t* __restrict__ place_ws,
                                                              int32_t* __restrict__ offsets) {
  const int lane = threadIdx.x;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  const bool live = active == nullptr || active[pr.p] != 0;
  int32_t* __restrict__ place = place_ws + pr.v0;
  int carry = 0;
  for (int i0 = 0; i0 < S; i0 += 64) {
    const int i = i0 + lane;
    int v = 0;
    if (i < S) v = 1 + (int)(live && pathq::inserts(pathq::unsafe(segment_max[pr.s0 + i], max_deviation), i, first_segment, S + 1));
    const int incl = wave_inclusive_sum(v, lane);
    if (i < S) place[i] = carry + incl - v;
    carry += __shfl(incl, 63);
  }
  if (lane == 0) {
    place[S] = carry;
    offsets[pr.p + 1] = carry + 1;
  }
}

__global__ __launch_bounds__(kPathEditScanChunk) void vertex_offsets_kernel(int n_paths, int32_t* __restrict__ offsets) {
  __shared__ int s_wave[kPathEditScanChunk / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;  // the same in every thread
  for (int p0 = 0; p0 < n_paths; p0 += kPathEditScanChunk) {
    const int p = p0 + tid;
    const int v = p < n_paths ? offsets[p + 1] : 0;
    const int incl = wave_inclusive_sum(v, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kPathEditScanChunk / 64; ++k) {
      const int t = s_wave[k];
      before += k < wave ? t : 0;
      total += t;
    }
    __syncthreads();  // (the next chunk overwrites the totals)
    if (p < n_paths) offsets[p + 1] = carry + before + incl;
    carry += total;
  }
  if (tid == 0) offsets[0] = 0;
}

template <bool kSubdivide>
__global__ __launch_bounds__(kWriteThreads) void edit_write_kernel(BatchView b, const double* __restrict__ waypoints,
                                                                   const uint8_t* __restrict__ stop_at,
                                                                   const int32_t* __restrict__ ws,
                                                                   const int32_t* __restrict__ offsets, int upper,
                                                                   double* __restrict__ waypoints_out,
                                                                   uint8_t* __restrict__ stop_out, int32_t* __restrict__ source_out,
                                                                   uint8_t* __restrict__ inserted_out) {
  const long long at = (long long)blockIdx.x * kWriteThreads + threadIdx.x;
  if (at >= (long long)upper) return;
  const int o = (int)at;
  if (o >= offsets[b.n_paths]) return;
  const int p = last_not_above(offsets, b.n_paths, o);
  const int j = o - offsets[p];
  const int s0 = first_segment(b, p);
  const int v0 = s0 + p;
  int i;
  bool mid = false;
  if (kSubdivide) {
    const int32_t* __restrict__ place = ws + v0;
    i = last_not_above(place, segments_of(b, p, s0) + 1, j);
    mid = place[i] != j;
  } else {
    i = ws[v0 + j];
  }
  const double* __restrict__ a = waypoints + (size_t)(v0 + i) * 4;
  double row[4];
  if (mid) {
    pathq::interpolate_point(a, a + 4, 0.5, row);
  } else {
    row[0] = a[0], row[1] = a[1], row[2] = a[2], row[3] = a[3];
  }
  row_pair* out = reinterpret_cast<row_pair*>(waypoints_out + (size_t)o * 4);
  row_pair lo, hi;
  lo.x = row[0], lo.y = row[1], hi.x = row[2], hi.y = row[3];
  out[0] = lo;
  out[1] = hi;
  if (stop_out) stop_out[o] = (mid || stop_at == nullptr) ? (uint8_t)0 : stop_at[v0 + i];
  if (source_out) source_out[o] = v0 + i;
  if (inserted_out) inserted_out[o] = mid ? 1 : 0;
}

__global__ __launch_bounds__(kWriteThreads) void path_edit_vjp_kernel(BatchView b, const int32_t* __restrict__ offsets,
                                                                      const int32_t* __restrict__ source,
                                                                      const uint8_t* __restrict__ inserted,
                                                                      const double* __restrict__ grad_edited,
                                                                      double* __restrict__ grad_waypoints) {
  const long long at = (long long)blockIdx.x * kWriteThreads + threadIdx.x;
  if (at >= (long long)b.n_segments + b.n_paths) return;
  const int v = (int)at;
  const int p = path_of_vertex(b, v);
  const int r0 = offsets[p], n_run = offsets[p + 1] - r0;
  double g[4];
  pathq::edit_gradient(source + r0, inserted ? inserted + r0 : nullptr, n_run, v, grad_edited + (size_t)r0 * 4, g);
  row_pair* out = reinterpret_cast<row_pair*>(grad_waypoints + (size_t)v * 4);
  row_pair lo, hi;
  lo.x = g[0], lo.y = g[1], hi.x = g[2], hi.y = g[3];
  out[0] = lo;
  out[1] = hi;
}

hipError_t launch_vertex_offsets(int n_paths, int32_t* offsets, hipEvent_t start, hipEvent_t stop, hipStream_t stream) {
  MRS_TG_LAUNCH_EXT(vertex_offsets_kernel, dim3(1), dim3(kPathEditScanChunk), 0, stream, start, stop, 0, n_paths, offsets);
  return hipGetLastError();
}

namespace {

// the launches behind the decision kernel: the offsets, then the rows; `kt` carries the call's timer from the first launch to the last
hipError_t finish_edit(bool subdivide, const BatchView& b, const KernelTimer& kt, bool first_launch, const double* waypoints,
                       const uint8_t* stop_at, const int32_t* ws, int upper, int32_t* offsets, double* waypoints_out,
                       uint8_t* stop_out, int32_t* source_out, uint8_t* inserted_out, hipStream_t stream) {
  const bool rows = b.n_paths > 0 && upper > 0;
  if (hipError_t e = launch_vertex_offsets(b.n_paths, offsets, first_launch ? kt.start : nullptr, rows ? nullptr : kt.stop, stream);
      e != hipSuccess)
    return e;
  if (!rows) return hipSuccess;
  const auto write = subdivide ? MRS_TG_KERNEL(edit_write_kernel<true>) : MRS_TG_KERNEL(edit_write_kernel<false>);
  MRS_TG_LAUNCH_EXT(write, dim3(cdiv(upper, kWriteThreads)), dim3(kWriteThreads), 0, stream, nullptr, kt.stop, 0, b, waypoints,
                    stop_at, ws, offsets, upper, waypoints_out, stop_out, source_out, inserted_out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_preprocess_path(const BatchView& b, const double* waypoints, const uint8_t* stop_at,
                                  const pathq::ThinOptions& o, int32_t* ws, int32_t* offsets, double* waypoints_out,
                                  uint8_t* stop_out, int32_t* source_out, hipStream_t stream) {
  const KernelTimer kt = take_kernel_timer();
  if (b.n_paths > 0) {
    MRS_TG_LAUNCH_EXT(thin_path_kernel, dim3((unsigned)b.n_paths), dim3(64), 0, stream, kt.start, nullptr, 0, b, waypoints, o, ws,
                      offsets);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return finish_edit(false, b, kt, b.n_paths <= 0, waypoints, stop_at, ws, b.n_segments + b.n_paths, offsets, waypoints_out,
                            stop_out, source_out, nullptr, stream);
}

hipError_t launch_insert_midpoints(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const double* segment_max,
                                   double max_deviation, int first_segment, const uint8_t* active, int32_t* ws, int32_t* offsets,
                                   double* waypoints_out, uint8_t* stop_out, int32_t* source_out, uint8_t* inserted_out,
                                   hipStream_t stream) {
  const KernelTimer kt = take_kernel_timer();
  if (b.n_paths > 0) {
    MRS_TG_LAUNCH_EXT(insert_midpoints_kernel, dim3((unsigned)b.n_paths), dim3(64), 0, stream, kt.start, nullptr, 0, b,
                      segment_max, max_deviation, first_segment, active, ws, offsets);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return finish_edit(true, b, kt, b.n_paths <= 0, waypoints, stop_at, ws, 2 * b.n_segments + b.n_paths, offsets, waypoints_out,
                           stop_out, source_out, inserted_out, stream);
}

hipError_t launch_path_edit_vjp(const BatchView& b, const int32_t* offsets, const int32_t* source, const uint8_t* inserted,
                                const double* grad_edited, double* grad_waypoints, hipStream_t stream) {
  if (b.n_paths <= 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(path_edit_vjp_kernel, dim3(cdiv((long long)b.n_segments + b.n_paths, kWriteThreads)), dim3(kWriteThreads),
                      0, stream, b, offsets, source, inserted, grad_edited, grad_waypoints);
  return hipGetLastError();
}

}  // namespace mrs_tg

// mrs_tg_heading.hip -- the heading along the direction of travel (mrs_tg_plan_travel_heading) and its backward pass
// (mrs_tg_plan_travel_heading_vjp); mrs_tg_heading.hpp, DESIGN.md section 11f.  The stage is getTrajectoryReference with
// override_heading_atan2: a row takes atan2 of the step to the next row, a row that barely moves the heading of the row in
// front -- which chains, so a row's heading is that of the highest SOURCE (a row that moves, or row 0) at or below it.
// ONE WAVEFRONT TAKES ONE PATH, ONE LANE ONE ROW of a chunk of 64.
//   travel_heading_kernel      one ballot gives the chunk's sources; a lane finds its own by a clz on the mask cut at its lane
//                              and takes the value by one shuffle; without a source at or below it in the chunk it takes what
//                              lane 63 of the chunk in front ended with.  A carried heading is a copy, never a second atan2.
//   travel_heading_vjp_kernel  finds the same sources; every source adds up the upstream of its run in increasing row index
//                              (the lanes walk their runs side by side, as many steps as the chunk's longest run has rows).
//                              The run of a chunk's last source goes on behind the chunk: the wavefront reads on, chunk after
//                              chunk, until it meets the next source, so that every lane knows its sum when it stores its row;
//                              a chunk is read at most twice.  The term a step gives the row behind it crosses the lanes by a
//                              shuffle and the chunks in two registers.
// Reads and register traffic only: no LDS, no atomics, no workspace; every output element is written once.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_heading.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

// (samples_out may be samples: then only the heading of the rows 0 .. n-2 is stored, and x, y, z are all that is read of them)
__global__ __launch_bounds__(64) void travel_heading_kernel(const double* samples, const int32_t* __restrict__ n_samples,
                                                            int capacity, const int32_t* __restrict__ status, double min_step,
                                                            double* samples_out, int32_t* __restrict__ source_out) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  if (n <= 0) return;
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* rows = samples + row0 * 4;
  double* out = samples_out + row0 * 4;
  const bool in_place = samples_out == samples;
  double cur[3];
  load_xyz(rows, lane, n, cur);
  double carry_h = 0.0;  // what the last row of the chunk in front ended with (row 0 is a source: never read in the first chunk)
  int carry_s = 0;
  for (int k0 = 0; k0 < n - 1; k0 += 64) {
    const int i = k0 + lane;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    seam_neighbour(cur, nxt, lane, nx);
    const bool has = i < n - 1;
    const hdg::Step st = hdg::step_xy(cur, nx);
    const bool src = has && hdg::is_source(i, st.dist, min_step);
    double h = 0.0;
    if (src) h = hdg::heading_of(st.dx, st.dy);
    const unsigned long long mask = __ballot(src);
    const unsigned long long below = mask & (~0ull >> (63 - lane));
    const int sl = below ? 63 - __clzll((long long)below) : 0;
    const double hv = __shfl(h, sl);
    const double val = below ? hv : carry_h;
    const int sidx = below ? k0 + sl : carry_s;
    if (has) {
      if (in_place) {
        out[(size_t)i * 4 + 3] = val;
      } else {
        row_pair* o = reinterpret_cast<row_pair*>(out + (size_t)i * 4);
        row_pair lo, hi;
        lo.x = cur[0], lo.y = cur[1], hi.x = cur[2], hi.y = val;
        o[0] = lo;
        o[1] = hi;
      }
      if (source_out) source_out[row0 + i] = sidx;
    }
    carry_h = __shfl(val, 63);
    carry_s = __shfl(sidx, 63);
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  if (lane == 0) {  // the last row keeps what it has
    if (!in_place) {
      const row_pair* r = reinterpret_cast<const row_pair*>(rows + (size_t)(n - 1) * 4);
      row_pair* o = reinterpret_cast<row_pair*>(out + (size_t)(n - 1) * 4);
      const row_pair lo = r[0], hi = r[1];
      o[0] = lo;
      o[1] = hi;
    }
    if (source_out) source_out[row0 + n - 1] = -1;
  }
}

__global__ __launch_bounds__(64) void travel_heading_vjp_kernel(const double* __restrict__ samples,
                                                                const int32_t* __restrict__ n_samples, int capacity,
                                                                const int32_t* __restrict__ status, double min_step,
                                                                const double* __restrict__ grad_out,
                                                                double* __restrict__ grad_samples) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const int n = live_samples(path_live(status, p), n_samples, p, capacity);
  const size_t row0 = (size_t)p * (size_t)capacity;
  const double* __restrict__ rows = samples + row0 * 4;
  const double* __restrict__ up = grad_out + row0 * 4;
  row_pair* __restrict__ gs = reinterpret_cast<row_pair*>(grad_samples + row0 * 4);
  double cur[3];
  load_xyz(rows, lane, n, cur);
  double carry_b[2] = {0.0, 0.0};  // what the step of the chunk's last row gives the first row of the next chunk
  bool carry_src = false;
  for (int k0 = 0; k0 < n - 1; k0 += 64) {
    const int i = k0 + lane;
    double nxt[3], nx[3];
    load_xyz(rows, i + 64, n, nxt);
    row_pair ulo, uhi;
    ulo.x = ulo.y = uhi.x = uhi.y = 0.0;
    if (i < n) {
      const row_pair* u = reinterpret_cast<const row_pair*>(up + (size_t)i * 4);
      ulo = u[0], uhi = u[1];
    }
    seam_neighbour(cur, nxt, lane, nx);
    const bool has = i < n - 1;
    const hdg::Step st = hdg::step_xy(cur, nx);
    const bool src = has && hdg::is_source(i, st.dist, min_step);
    const double g3 = has ? uhi.y : 0.0;
    const unsigned long long mask = __ballot(src);
    const int count = min(64, n - 1 - k0);
    // a source's run inside the chunk: up to the next source or the chunk's last row with a step
    const unsigned long long above = lane == 63 ? 0ull : mask & (~0ull << (lane + 1));
    const int e = above ? __ffsll((long long)above) - 1 : count;
    const int len = src ? e - lane : 0;
    double G = 0.0;
    for (int t = 0; __ballot(t < len) != 0; ++t) {
      const double v = __shfl(g3, (lane + t) & 63);
      if (t < len) G = hdg::accumulate(G, v);
    }
    if (mask != 0 && k0 + 64 < n - 1) {  // the last source's run goes on behind the chunk, up to the next source
      const int last = 63 - __clzll((long long)mask);
      double acc = __shfl(G, last);
      for (int k1 = k0 + 64; k1 < n - 1; k1 += 64) {
        const int i2 = k1 + lane;
        bool src2 = false;
        double g2 = 0.0;
        if (i2 < n - 1) {
          const hdg::Step s2 = hdg::step_xy(rows + (size_t)i2 * 4, rows + (size_t)i2 * 4 + 4);
          src2 = hdg::is_source(i2, s2.dist, min_step);
          g2 = up[(size_t)i2 * 4 + 3];
        }
        const unsigned long long mask2 = __ballot(src2);
        const int count2 = mask2 ? __ffsll((long long)mask2) - 1 : min(64, n - 1 - k1);
        for (int t = 0; t < count2; ++t) acc = hdg::accumulate(acc, __shfl(g2, t));
        if (mask2) break;
      }
      if (lane == last) G = acc;
    }
    double ra[2] = {0.0, 0.0}, rb[2] = {0.0, 0.0};
    if (src) hdg::atan2_rows(st.dx, st.dy, G, ra, rb);
    double pbx = __shfl_up(rb[0], 1), pby = __shfl_up(rb[1], 1);
    bool psrc = __shfl_up((int)src, 1) != 0;
    if (lane == 0) pbx = carry_b[0], pby = carry_b[1], psrc = carry_src;
    double x = ulo.x, y = ulo.y;
    if (src) x = hdg::accumulate(x, ra[0]), y = hdg::accumulate(y, ra[1]);
    if (psrc) x = hdg::accumulate(x, pbx), y = hdg::accumulate(y, pby);
    if (i < n) {
      row_pair lo, hi;
      lo.x = x, lo.y = y, hi.x = uhi.x, hi.y = i == n - 1 ? uhi.y : 0.0;
      gs[2 * (size_t)i] = lo;
      gs[2 * (size_t)i + 1] = hi;
    }
    carry_b[0] = __shfl(rb[0], 63), carry_b[1] = __shfl(rb[1], 63);
    carry_src = __shfl((int)src, 63) != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) cur[k] = nxt[k];
  }
  if (n >= 1 && (n - 1) % 64 == 0 && lane == 0) {  // the last row where no chunk reached it
    const row_pair* u = reinterpret_cast<const row_pair*>(up + (size_t)(n - 1) * 4);
    row_pair lo = u[0];
    const row_pair hi = u[1];
    if (carry_src) lo.x = hdg::accumulate(lo.x, carry_b[0]), lo.y = hdg::accumulate(lo.y, carry_b[1]);
    gs[2 * (size_t)(n - 1)] = lo;
    gs[2 * (size_t)(n - 1) + 1] = hi;
  }
  row_pair zero;
  zero.x = 0.0, zero.y = 0.0;
  for (size_t e = 2 * (size_t)n + lane; e < 2 * (size_t)capacity; e += 64) gs[e] = zero;
}

hipError_t launch_travel_heading(int n_paths, const double* samples, const int32_t* n_samples, int capacity, const int32_t* status,
                                 double min_step, double* samples_out, int32_t* source_out, hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(travel_heading_kernel, dim3((unsigned)n_paths), dim3(64), 0, stream, samples, n_samples, capacity, status,
                      min_step, samples_out, source_out);
  return hipGetLastError();
}

hipError_t launch_travel_heading_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                     const int32_t* status, double min_step, const double* grad_out, double* grad_samples,
                                     hipStream_t stream) {
  if (n_paths == 0 || capacity == 0) return hipSuccess;
  MRS_TG_LAUNCH_TIMED(travel_heading_vjp_kernel, dim3((unsigned)n_paths), dim3(64), 0, stream, samples, n_samples, capacity,
                      status, min_step, grad_out, grad_samples);
  return hipGetLastError();
}

}  // namespace mrs_tg

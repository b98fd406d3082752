// mrs_tg_pathwave.hpp -- what the kernels that give ONE WAVEFRONT ONE PATH share around their own loops (mrs_tg_sample_vjp.hip,
// mrs_tg_evaluate.hip, mrs_tg_deviation.hip, mrs_tg_passage.hip, mrs_tg_heading.hip, mrs_tg_pathedit.hip, mrs_tg_initial.hip).  Device only; only what they spell the same way AND compile
// to the same code through a function: the chunk loops and the loops that stage a path into LDS stay written out.
// The kernels that give ONE WORKGROUP ONE PATH (mrs_tg_clearance.hip, mrs_tg_obstacle.hip, mrs_tg_field.hip) take the row helpers
// from here too, and the end they share: write_path_minimum.
#pragma once
#include "mrs_tg_clearance.hpp"
#include "mrs_tg_device.hpp"

namespace mrs_tg {

// two doubles as one 16-byte word: half a row [4]
typedef double row_pair __attribute__((ext_vector_type(2)));

// a path the solve gave up on (status <= 0; no status: every path is live) contributes nothing, whatever its arrays hold
__device__ __forceinline__ bool path_live(const int32_t* status, int p) { return status == nullptr || status[p] > 0; }
// ... and has no samples; a live one has as many as it reports, at most the capacity
__device__ __forceinline__ int live_samples(bool live, const int32_t* n_samples, int p, int capacity) {
  const int n = live ? min(n_samples[p], capacity) : 0;
  return n < 0 ? 0 : n;
}

// the largest p in [0, n) with first[p] <= x (first non-decreasing, first[0] <= x): the path of an element of a packed batch from
// the batch's offsets, a path without elements never being the answer for an element of a path behind it
__device__ __forceinline__ int last_not_above(const int32_t* __restrict__ first, int n, int x) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// x, y, z of row i of [n][4] rows (zeros behind them)
__device__ __forceinline__ void load_xyz(const double* __restrict__ rows, int i, int n, double (&s)[3]) {
  s[0] = s[1] = s[2] = 0.0;
  if (i < n) {
    const row_pair* __restrict__ r = reinterpret_cast<const row_pair*>(rows + (size_t)i * 4);
    const row_pair lo = r[0];
    s[0] = lo.x, s[1] = lo.y, s[2] = rows[(size_t)i * 4 + 2];
  }
}

// the row behind every lane's own: the next lane's, and for lane 63 the first of the next chunk (the seam)
__device__ __forceinline__ void seam_neighbour(const double (&cur)[3], const double (&nxt)[3], int lane, double (&nx)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double down = __shfl_down(cur[k], 1);
    const double seam = __shfl(nxt[k], 0);
    nx[k] = lane == 63 ? seam : down;
  }
}

// (x, y, z, 0) as the row [4] at `row`: two 16-byte words
__device__ __forceinline__ void store_xyz0(double* __restrict__ row, const double (&v)[3]) {
  row_pair* out = reinterpret_cast<row_pair*>(row);
  row_pair lo, hi;
  lo.x = v[0], lo.y = v[1], hi.x = v[2], hi.y = 0.0;
  out[0] = lo;
  out[1] = hi;
}

// The minimum of a path whose rows ONE WORKGROUP of kWaves wavefronts shares: every lane brings the first smallest of its rows as
// best = (c, row) and tag -- what the step records beside the row: partner, obstacle, cell.  Combined in clrq::better's order
// "smaller value, then lower row" by shuffles and, across the wavefronts, through kWaves LDS slots; the order is free of how the
// rows were dealt, so the split changes no bit.  Thread 0 writes min_clearance[p] and argmin[2p], argmin[2p + 1]; nothing where
// the caller wants neither.  Every thread of the workgroup calls it (one barrier).  `best` whole and by value: the spelling
// whose code is nearest the kernels' own copies (profiles/clearance_family_isa_identity.txt).
template <int kWaves>
__device__ __forceinline__ void write_path_minimum(clrq::Nearest best, int tag, int lane, int wave, int p,
                                                   double* __restrict__ min_clearance, int32_t* __restrict__ argmin) {
  __shared__ double s_c[kWaves];
  __shared__ int s_row[kWaves], s_tag[kWaves];
  if (!min_clearance && !argmin) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double oc = __shfl_xor(best.c, o);
    const int orow = __shfl_xor(best.index, o), otag = __shfl_xor(tag, o);
    if (clrq::better(oc, orow, best.c, best.index)) best.c = oc, best.index = orow, tag = otag;
  }
  if (lane == 0) s_c[wave] = best.c, s_row[wave] = best.index, s_tag[wave] = tag;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWaves; ++w)
      if (clrq::better(s_c[w], s_row[w], best.c, best.index)) best.c = s_c[w], best.index = s_row[w], tag = s_tag[w];
    if (min_clearance) min_clearance[p] = best.c;
    if (argmin) argmin[2 * (size_t)p] = best.index, argmin[2 * (size_t)p + 1] = tag;
  }
}

// dL/dT_i = -(s_{i+1} + (s_{i+2} + ...)) of a path from its time sums s_i = s_sum[i * stride] in LDS (sampvjp::time_gradients'
// order), lane 0 writing grad_times[s0 + i] of the batch's array; nothing without grad_times
__device__ __forceinline__ void write_time_gradients(const double* s_sum, int stride, int s0, int S, int lane, double* grad_times) {
  if (!grad_times) return;
  double r = 0.0;
  for (int i = S - 1; i >= 0; --i) {
    if (lane == 0) grad_times[s0 + i] = 0.0 - r;
    r = accumulate(s_sum[i * stride], r);
  }
}

}  // namespace mrs_tg

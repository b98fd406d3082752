// mrs_tg_sample_vjp.hip -- the backward pass of the sampler (mrs_tg_plan_sample_states_vjp; mrs_tg_sample_vjp.hpp, DESIGN.md
// section 7b): from dL/dsamples, the gradients with respect to the coefficients and the segment times, and the (segment,
// time) every sample was taken at.  One wavefront per path, as sample_kernel: times and coefficients staged in LDS, the walk
// is the forward's own (sample_path_walk with this file's consumer at each flush).  At a flush the parked samples are visited
// in increasing index with LANE = OUTPUT ELEMENT: lanes 0..39 hold dL/dc[dim][j] of the current segment, lanes 40..40+4 NO-1
// the (o, dim) partial of its time sum; the walk is monotone, so a segment's accumulators are written once, when the segment
// index changes or the walk ends.  Reads only; no atomics, every output element written exactly once: two calls give the same
// bits, and no sum depends on the chunking of the walk.
#include <hip/hip_runtime.h>

#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"
#include "mrs_tg_sample_vjp.hpp"
#include "mrs_tg_sampling.hpp"

namespace mrs_tg {

namespace {

constexpr int kSvLoadAhead = 4;  // samples whose upstream rows are requested before the first of them is consumed: the
                                 // loads of a group are in flight before the stores of a finished segment are issued
                                 // (gfx950 counts loads and stores in one in-order counter)

template <int NO>
struct SampleVjpSink {
  int lane, role;  // role 0: coefficient element (dim, j); 1: time partial (o, dim); 2: idle
  int dim, j, o;
  int ofs[NO];     // which entries of a sample's upstream row [NO][4] this lane reads
  double w[sampvjp::kN];
  const double* s_c;     // LDS: the path's coefficients [S][4][10]
  double* s_sum;         // LDS: the time sum s_i of every segment [S]
  const double* G;       // the path's upstream rows [capacity][NO][4]; null = no gradient is accumulated
  double* gc;            // the path's dL/dc [S][40] or null
  bool want_times;
  bool active;           // false: the walk only counts (sample_path_walk)
  int32_t* seg_out;      // the path's [capacity] or null
  double* time_out;
  int cur = -1;          // the segment the accumulators belong to
  double acc = 0.0;

  __device__ __forceinline__ void init(int lane_, bool want_times_) {
    lane = lane_;
    want_times = want_times_;
    const int r = lane - sampvjp::kCoeffElems;
    role = lane < sampvjp::kCoeffElems ? 0 : (want_times && r < NO * sampvjp::kD ? 1 : 2);
    if (role == 1) {
      o = r / sampvjp::kD, dim = r % sampvjp::kD, j = 0;
      sampvjp::time_weights(o, w);
#pragma unroll
      for (int q = 0; q < NO; ++q) ofs[q] = r;
    } else {
      const int e = role == 0 ? lane : 0;  // (idle lanes run element 0's arithmetic and store nothing)
      dim = e / sampvjp::kN, j = e % sampvjp::kN, o = 0;
      sampvjp::coeff_weights(j, w);
#pragma unroll
      for (int q = 0; q < NO; ++q) ofs[q] = q * sampvjp::kD + dim;
    }
  }

  // the accumulators of segment `cur` leave; the segments [cur + 1, next) hold no sample: zero rows
  __device__ __forceinline__ void close_segments(int next) {
    if (cur >= 0) {
      if (gc && role == 0) gc[(size_t)cur * sampvjp::kCoeffElems + lane] = acc;
      if (want_times) {
        double s = lane_value(acc, sampvjp::kCoeffElems);
#pragma unroll
        for (int r = 1; r < NO * sampvjp::kD; ++r) s = sampvjp::accumulate(s, lane_value(acc, sampvjp::kCoeffElems + r));
        if (lane == 0) s_sum[cur] = s;
      }
    }
    for (int i = cur + 1; i < next; ++i) {
      if (gc && role == 0) gc[(size_t)i * sampvjp::kCoeffElems + lane] = 0.0;
      if (want_times && lane == 0) s_sum[i] = 0.0;
    }
  }

  // sample_path_walk's consumer: the parked samples [first, first + count) of the path (below the capacity)
  __device__ __forceinline__ void flush(const double* s_t, const unsigned short* s_seg, int first, int count) {
    for (int e = lane; e < count; e += 64) {
      if (seg_out) seg_out[first + e] = (int32_t)s_seg[e];
      if (time_out) time_out[first + e] = s_t[e];
    }
    if (!G) return;
    for (int e0 = 0; e0 < count; e0 += kSvLoadAhead) {
      double g[kSvLoadAhead][NO];
#pragma unroll
      for (int u = 0; u < kSvLoadAhead; ++u) {
        const int e = min(e0 + u, count - 1);  // (a group's tail reads the last sample's row again: never a row beyond it)
        const double* __restrict__ row = G + (size_t)(first + e) * (NO * sampvjp::kD);
#pragma unroll
        for (int q = 0; q < NO; ++q) g[u][q] = row[ofs[q]];
      }
#pragma unroll
      for (int u = 0; u < kSvLoadAhead; ++u) {
        if (e0 + u >= count) break;
        const int seg = __builtin_amdgcn_readfirstlane((int)s_seg[e0 + u]);
        const double t = s_t[e0 + u];
        if (seg != cur) {
          close_segments(seg);
          cur = seg;
          acc = 0.0;
        }
        double term;
        if (role == 1)
          term = sampvjp::time_term(o, w, s_c + (size_t)seg * sampvjp::kCoeffElems + dim * sampvjp::kN, g[u][0], t);
        else
          term = sampvjp::coeff_term<NO>(j, w, g[u], t);
        acc = sampvjp::accumulate(acc, term);
      }
    }
  }
};

}  // namespace

template <int NO>
__global__ __launch_bounds__(64) void sample_vjp_kernel(BatchView b, const double* __restrict__ coeffs,
                                                        const double* __restrict__ seg_times, double dt, int capacity,
                                                        const double* __restrict__ grad_states,
                                                        const int32_t* __restrict__ status, double* __restrict__ grad_coeffs,
                                                        double* __restrict__ grad_times, int32_t* __restrict__ sample_segment,
                                                        double* __restrict__ sample_time, int32_t* __restrict__ n_samples,
                                                        const double* __restrict__ acc_table, int acc_n) {
  // [max_segments] segment times | [S][4][10] coefficients | [max_segments] time sums | sample buffer
  extern __shared__ double s_T[];
  const int lane = threadIdx.x;
  double* s_c = s_T + b.max_segments;
  double* s_sum = s_c + (size_t)b.max_segments * kD * kN;
  double* s_t = s_sum + b.max_segments;
  unsigned short* s_seg = reinterpret_cast<unsigned short*>(s_t + kSampleBuffer);
  const bool want_grad = grad_coeffs != nullptr || grad_times != nullptr;
  for (int q = blockIdx.x; q < b.n_paths; q += gridDim.x) {
    const PathRef pr = path_at(b, q);
    const int S = pr.S;
    // a path the solve gave up on contributes nothing, whatever its coefficients hold
    // (path_live of mrs_tg_pathwave.hpp, written out: through the function the compiler swaps the operands of this conjunction)
    const bool live = want_grad && (status == nullptr || status[pr.p] > 0);
    for (int i = lane; i < S; i += 64) s_T[i] = seg_times[pr.s0 + i];
    if (live && grad_times) {  // (only the time partials read coefficients)
      const double* __restrict__ cg = coeffs + (size_t)pr.s0 * kD * kN;
      for (int e = lane; e < S * kD * kN; e += 64) s_c[e] = cg[e];
    }
    __syncthreads();
    SampleVjpSink<NO> sink;
    sink.init(lane, grad_times != nullptr);
    sink.s_c = s_c;
    sink.s_sum = s_sum;
    sink.G = live ? grad_states + (size_t)pr.p * capacity * (NO * kD) : nullptr;
    sink.gc = grad_coeffs ? grad_coeffs + (size_t)pr.s0 * kD * kN : nullptr;
    sink.seg_out = sample_segment ? sample_segment + (size_t)pr.p * capacity : nullptr;
    sink.time_out = sample_time ? sample_time + (size_t)pr.p * capacity : nullptr;
    sink.active = capacity > 0 && (sink.G || sink.seg_out || sink.time_out);
    const int n = sample_path_walk<0, SampleVjpSink<NO>>(s_T, s_c, s_t, s_seg, S, dt, capacity, nullptr, acc_table, acc_n,
                                                         &sink);
    if (lane == 0 && n_samples) n_samples[pr.p] = n;
    if (want_grad) {
      sink.close_segments(S);  // the last segment with samples, and zero rows for every segment behind it
      if (grad_times) {
        wave_lds_barrier();
        write_time_gradients(s_sum, 1, pr.s0, S, lane, grad_times);
      }
    }
    __syncthreads();  // (the next path's staging overwrites what this walk read)
  }
}

hipError_t launch_sample_vjp(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                             int n_orders, const double* grad_states, const int32_t* status, double* grad_coeffs,
                             double* grad_times, int32_t* sample_segment, double* sample_time, int32_t* n_samples,
                             hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  if (!valid_state_orders(n_orders)) return hipErrorInvalidValue;
  const double* acc_table = nullptr;
  int acc_n = 0;
  AccPin pin;  // (released when this function returns: behind the enqueue of the kernel that reads the table)
  if (!dry_run()) {
    hipError_t et = sample_acc_table(dt, capacity, stream, &acc_table, &acc_n, &pin);
    if (et != hipSuccess) return et;
  }
  const size_t lds = sizeof(double) * ((size_t)b.max_segments * (2 + kD * kN) + kSampleBuffer) + sizeof(unsigned short) * kSampleBuffer;
  const auto vjp = n_orders == 1 ? MRS_TG_KERNEL(sample_vjp_kernel<1>) : MRS_TG_KERNEL(sample_vjp_kernel<kSampleStateOrders>);
  if (hipError_t e = prepare_dynamic_lds(vjp, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(vjp, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, coeffs, seg_times, dt, capacity, grad_states, status,
                      grad_coeffs, grad_times, sample_segment, sample_time, n_samples, acc_table, acc_n);
  return hipGetLastError();
}

}  // namespace mrs_tg

// mrs_tg_evaluate.hip -- the state of every path at caller-given times (mrs_tg_plan_evaluate) and its backward pass
// (mrs_tg_plan_evaluate_vjp); mrs_tg_evaluate.hpp, DESIGN.md section 7c.  Nothing here is serial in the queries: the segment
// times, their running sums and the coefficients of a path are staged in LDS, and ONE LANE TAKES ONE QUERY -- it finds its
// segment among the sums (Trajectory::evaluate's rule) and runs the Horner chains of its state row, or of its terms of the
// gradients.
//   evaluate_kernel      one wavefront per (path, slice of its queries); streaming stores, as the sampler's flush -- with five
//                        orders the 64 rows of a pass go through LDS, so that every store instruction writes 1 KB without a gap.
//   evaluate_vjp_kernel  one wavefront per path.  64 queries per pass: every lane forms the 40 coefficient terms and the
//                        time gradient g of its query in registers; the terms are then parked, 32 queries at a time, in an
//                        LDS tile [query][41] and summed with LANE = OUTPUT ELEMENT, one query per step (one LDS read and one
//                        addition): the accumulator of the current segment lives in a register and changes places with the
//                        path's LDS accumulators [S][41] only when the segment changes.  Every sum over a segment's queries
//                        therefore runs in increasing query index from 0.0, whatever the order of the queries and wherever
//                        the passes cut them.  Reads only; no atomics, every output element written exactly once.
#include <hip/hip_runtime.h>

#include "mrs_tg_device.hpp"
#include "mrs_tg_evaluate.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pathwave.hpp"

namespace mrs_tg {

namespace {

constexpr int kEvTileQueries = 32;                       // queries parked per reduction step of the backward pass
constexpr int kEvTileStride = evalq::kCoeffElems + 1;    // 40 coefficient terms + the time gradient
constexpr int kEvRowStride = 21;                         // doubles between the rows [5][4] of a pass in LDS (odd: no bank is hit 8 times)
constexpr int kEvTargetBlocks = 8192;                    // the forward cuts the queries of few paths into slices up to here

}  // namespace

template <int NO>
__global__ __launch_bounds__(64) void evaluate_kernel(BatchView b, const double* __restrict__ coeffs,
                                                      const double* __restrict__ seg_times,
                                                      const double* __restrict__ query_times, int n_queries, int slice,
                                                      double* __restrict__ states, int32_t* __restrict__ query_segment,
                                                      double* __restrict__ query_tau) {
  // [max_segments] segment times | [max_segments] running sums | [max_segments][4][10] coefficients | NO = 5: [64][21] rows
  extern __shared__ double s_T[];
  const int lane = threadIdx.x;
  double* s_A = s_T + b.max_segments;
  double* s_c = s_A + b.max_segments;
  const PathRef pr = path_at(b, blockIdx.x);
  const int S = pr.S;
  for (int i = lane; i < S; i += 64) s_T[i] = seg_times[pr.s0 + i];
  {
    const double* __restrict__ cg = coeffs + (size_t)pr.s0 * kD * kN;
    for (int e = lane; e < S * kD * kN; e += 64) s_c[e] = cg[e];
  }
  wave_lds_barrier();
  const bool sorted = evalq::running_sums(s_T, S, s_A, lane == 0);
  wave_lds_barrier();
  const int k_begin = blockIdx.y * slice;
  const int k_end = min(k_begin + slice, n_queries);
  const size_t row0 = (size_t)pr.p * (size_t)n_queries;
  constexpr int kRow = NO * kD;
  for (int k0 = k_begin; k0 < k_end; k0 += 64) {
    const int k = k0 + lane;
    const bool valid = k < k_end;
    evalq::Located at;
    at.seg = -1, at.tau = 0.0;
    if (valid) at = evalq::locate(s_T, s_A, S, sorted, __builtin_nontemporal_load(query_times + row0 + k));
    double row[NO][kD];
    if (at.seg >= 0) {
      evalq::state_row<NO>(s_c + (size_t)at.seg * (kD * kN), at.tau, row);
    } else {
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int dd = 0; dd < kD; ++dd) row[o][dd] = 0.0;
    }
    if constexpr (NO == 1) {  // 32 bytes per lane: two stores of the wavefront cover 2 KB without a gap
      if (valid) {
        row_pair* out = reinterpret_cast<row_pair*>(states + (row0 + k) * (size_t)kRow);
        row_pair lo, hi;
        lo.x = row[0][0], lo.y = row[0][1], hi.x = row[0][2], hi.y = row[0][3];
        __builtin_nontemporal_store(lo, out);
        __builtin_nontemporal_store(hi, out + 1);
      }
    } else {
      // 160 bytes per lane: stored from the lanes' registers, one store instruction would touch 64 lines 16 bytes each.  The
      // rows of a pass are contiguous in memory (10 KB), so they change places in LDS and every store of the wavefront
      // writes 1 KB without a gap.
      double* s_rows = s_c + (size_t)b.max_segments * kD * kN;
      double* mine = s_rows + lane * kEvRowStride;
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int dd = 0; dd < kD; ++dd) mine[o * kD + dd] = row[o][dd];
      wave_lds_barrier();
      const int pairs = min(64, k_end - k0) * (kRow / 2);
      row_pair* out = reinterpret_cast<row_pair*>(states + (row0 + k0) * (size_t)kRow);
#pragma unroll
      for (int i = 0; i < kRow / 2; ++i) {
        const int ch = lane + 64 * i;
        if (ch < pairs) {
          const double* src = s_rows + (ch / (kRow / 2)) * kEvRowStride + (ch % (kRow / 2)) * 2;
          row_pair v;
          v.x = src[0], v.y = src[1];
          __builtin_nontemporal_store(v, out + ch);
        }
      }
      wave_lds_barrier();  // (the next pass overwrites the rows)
    }
    if (valid) {
      if (query_segment) __builtin_nontemporal_store((int32_t)at.seg, query_segment + row0 + k);
      if (query_tau) __builtin_nontemporal_store(at.tau, query_tau + row0 + k);
    }
  }
}

template <int NO>
__global__ __launch_bounds__(64) void evaluate_vjp_kernel(BatchView b, const double* __restrict__ coeffs,
                                                          const double* __restrict__ seg_times,
                                                          const double* __restrict__ query_times, int n_queries,
                                                          const double* __restrict__ grad_states,
                                                          const int32_t* __restrict__ status, double* __restrict__ grad_coeffs,
                                                          double* __restrict__ grad_times, double* __restrict__ grad_query) {
  // [max_segments] times | [max_segments] running sums | [S][4][10] coefficients | [S][41] accumulators | [32][41] tile |
  // [32] segments of the parked queries
  extern __shared__ double s_T[];
  const int lane = threadIdx.x;
  double* s_A = s_T + b.max_segments;
  double* s_c = s_A + b.max_segments;
  double* s_acc = s_c + (size_t)b.max_segments * kD * kN;
  double* s_tile = s_acc + (size_t)b.max_segments * kEvTileStride;
  int* s_seg = reinterpret_cast<int*>(s_tile + kEvTileQueries * kEvTileStride);
  const bool want_time = grad_times != nullptr || grad_query != nullptr;
  const int slot = min(lane, kEvTileStride - 1);  // (lanes beyond the 41 output elements run the last one's and store nothing)
  const bool owns = lane < kEvTileStride;
  for (int q = blockIdx.x; q < b.n_paths; q += gridDim.x) {
    const PathRef pr = path_at(b, q);
    const int S = pr.S;
    // a path the solve gave up on contributes nothing, whatever its coefficients hold
    const bool live = path_live(status, pr.p);
    const size_t row0 = (size_t)pr.p * (size_t)n_queries;
    for (int i = lane; i < S; i += 64) s_T[i] = seg_times[pr.s0 + i];
    if (live && want_time) {  // (only the time gradients read coefficients)
      const double* __restrict__ cg = coeffs + (size_t)pr.s0 * kD * kN;
      for (int e = lane; e < S * kD * kN; e += 64) s_c[e] = cg[e];
    }
    for (int e = lane; e < S * kEvTileStride; e += 64) s_acc[e] = 0.0;
    wave_lds_barrier();
    const bool sorted = evalq::running_sums(s_T, S, s_A, lane == 0);
    wave_lds_barrier();
    int cur = -1;  // the segment the register accumulator belongs to
    double acc = 0.0;
    for (int k0 = 0; k0 < n_queries; k0 += 64) {
      const int k = k0 + lane;
      const bool valid = k < n_queries;
      if (!live) {
        if (grad_query && valid) grad_query[row0 + k] = 0.0;
        continue;
      }
      evalq::Located at;
      at.seg = -1, at.tau = 0.0;
      if (valid) at = evalq::locate(s_T, s_A, S, sorted, __builtin_nontemporal_load(query_times + row0 + k));
      double terms[evalq::kCoeffElems];
      double g = 0.0;
      if (at.seg >= 0) {  // (the upstream row of an out-of-range query is never read)
        double G[NO * kD];
        const row_pair* __restrict__ up = reinterpret_cast<const row_pair*>(grad_states + (row0 + k) * (size_t)(NO * kD));
#pragma unroll
        for (int e = 0; e < NO * kD / 2; ++e) {
          const row_pair v = __builtin_nontemporal_load(up + e);
          G[2 * e] = v.x, G[2 * e + 1] = v.y;
        }
        evalq::coeff_terms<NO>(G, at.tau, terms);
        if (want_time) g = evalq::time_gradient<NO>(s_c + (size_t)at.seg * (kD * kN), G, at.tau);
      } else {
#pragma unroll
        for (int e = 0; e < evalq::kCoeffElems; ++e) terms[e] = 0.0;
      }
      if (grad_query && valid) grad_query[row0 + k] = g;
#pragma unroll
      for (int h = 0; h < 64 / kEvTileQueries; ++h) {
        const int count = min(kEvTileQueries, n_queries - k0 - h * kEvTileQueries);
        if (count <= 0) break;
        if (lane / kEvTileQueries == h) {
          double* mine = s_tile + (lane % kEvTileQueries) * kEvTileStride;
#pragma unroll
          for (int e = 0; e < evalq::kCoeffElems; ++e) mine[e] = terms[e];
          mine[evalq::kCoeffElems] = g;
          s_seg[lane % kEvTileQueries] = at.seg;
        }
        wave_lds_barrier();
        for (int r = 0; r < count; ++r) {
          const int seg = __builtin_amdgcn_readfirstlane(s_seg[r]);
          if (seg < 0) continue;
          if (seg != cur) {
            if (cur >= 0 && owns) s_acc[cur * kEvTileStride + slot] = acc;
            acc = s_acc[seg * kEvTileStride + slot];
            cur = seg;
          }
          acc = sampvjp::accumulate(acc, s_tile[r * kEvTileStride + slot]);
        }
        wave_lds_barrier();
      }
    }
    if (cur >= 0 && owns) s_acc[cur * kEvTileStride + slot] = acc;
    wave_lds_barrier();
    if (grad_coeffs) {
      double* __restrict__ gc = grad_coeffs + (size_t)pr.s0 * kD * kN;
      for (int e = lane; e < S * kD * kN; e += 64) gc[e] = s_acc[(e / evalq::kCoeffElems) * kEvTileStride + e % evalq::kCoeffElems];
    }
    write_time_gradients(s_acc + evalq::kCoeffElems, kEvTileStride, pr.s0, S, lane, grad_times);
    wave_lds_barrier();  // (the next path's staging overwrites what this one read)
  }
}

hipError_t launch_evaluate(const BatchView& b, const double* coeffs, const double* seg_times, const double* query_times,
                           int n_queries, int n_orders, double* states, int32_t* query_segment, double* query_tau,
                           hipStream_t stream) {
  if (!valid_state_orders(n_orders)) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * ((size_t)b.max_segments * (2 + kD * kN) + (n_orders == 1 ? 0 : 64 * kEvRowStride));
  if (b.n_paths == 0 || n_queries == 0) return empty_batch_lds(lds);
  const auto fwd = n_orders == 1 ? MRS_TG_KERNEL(evaluate_kernel<1>) : MRS_TG_KERNEL(evaluate_kernel<kSampleStateOrders>);
  if (hipError_t e = prepare_dynamic_lds(fwd, lds); e != hipSuccess) return e;
  // one wavefront per path; the queries of few paths are cut into slices (multiples of 64) so that the device has work
  const int passes = (n_queries + 63) / 64;
  int slices = (kEvTargetBlocks + b.n_paths - 1) / b.n_paths;
  slices = slices < 1 ? 1 : (slices > passes ? passes : slices);
  const int slice = 64 * ((passes + slices - 1) / slices);
  slices = (n_queries + slice - 1) / slice;
  MRS_TG_LAUNCH_TIMED(fwd, dim3((unsigned)b.n_paths, (unsigned)slices), dim3(64), lds, stream, b, coeffs, seg_times, query_times,
                      n_queries, slice, states, query_segment, query_tau);
  return hipGetLastError();
}

hipError_t launch_evaluate_vjp(const BatchView& b, const double* coeffs, const double* seg_times, const double* query_times,
                               int n_queries, int n_orders, const double* grad_states, const int32_t* status,
                               double* grad_coeffs, double* grad_times, double* grad_query, hipStream_t stream) {
  if (!valid_state_orders(n_orders)) return hipErrorInvalidValue;
  const size_t lds = sizeof(double) * ((size_t)b.max_segments * (2 + kD * kN + kEvTileStride) + kEvTileQueries * kEvTileStride) +
                     sizeof(int) * kEvTileQueries;
  if (b.n_paths == 0) return empty_batch_lds(lds);
  const auto vjp = n_orders == 1 ? MRS_TG_KERNEL(evaluate_vjp_kernel<1>) : MRS_TG_KERNEL(evaluate_vjp_kernel<kSampleStateOrders>);
  if (hipError_t e = prepare_dynamic_lds(vjp, lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(vjp, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, coeffs, seg_times, query_times, n_queries,
                      grad_states, status, grad_coeffs, grad_times, grad_query);
  return hipGetLastError();
}

}  // namespace mrs_tg

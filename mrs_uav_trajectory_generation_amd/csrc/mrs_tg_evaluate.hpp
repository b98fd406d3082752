// mrs_tg_evaluate.hpp -- the state of a trajectory at a caller-given time (mrs_tg_plan_evaluate, evaluate_kernel) and one
// query's share of its backward pass (mrs_tg_plan_evaluate_vjp, evaluate_vjp_kernel); DESIGN.md section 7c.
//
// Locating the query t on a path with the segment times T_0 .. T_{S-1} is Trajectory::evaluate's rule: A_i = the running sum
// ((0 + T_0) + T_1) + ... + T_i, the segment is the first i with A_i > t (a query on a vertex belongs to the segment on its
// right, zero-length segments are skipped), S - 1 when there is none and t == A_{S-1}; start = A_i - T_i, computed like
// that, and tau = t - start.  Out of range (segment -1, tau 0, a zero state row): t < 0, t > A_{S-1}, t not a number, A_{S-1}
// not a number.
//   state[q][o][dim] = sum_{j >= o} j!/(j-o)! c[i][dim][j] tau^(j-o), Horner from j = 9 down (the heading of order 0 wrapped)
// Backward, with the upstream G[q][o][dim] and the membership held fixed:
//   dL/dc[i][dim][j] = sum over the in-range queries of segment i, in increasing q from 0.0, of sampvjp::coeff_term
//   g_q = dL/dt_q    = the sampvjp::time_terms G[q][o][dim] p_dim^(o+1)(tau) added in the order o * 4 + dim
//   s_i              = sum over the in-range queries of segment i, in increasing q from 0.0, of g_q
//   dL/dT_m          = -(s_{m+1} + (s_{m+2} + ( ... + s_{S-1})))                                    (sampvjp::time_gradients)
// Plain double, __host__ __device__ (tests/host/evaluate_harness.cpp runs it on the CPU): every product that could fuse is an
// explicit fma or kept apart by contraction being off, so the CPU and the GPU execute the same operations.
#pragma once

#include "mrs_tg_sample_vjp.hpp"

namespace mrs_tg {
namespace evalq {

using mrs_tg::kD;
using mrs_tg::kMaxOrders;
using mrs_tg::kN;
constexpr int kCoeffElems = sampvjp::kCoeffElems;

// A[i] = ((0 + T_0) + T_1) + ... + T_i, the additions of the reference's loop.  Returns whether the sums never decrease (no
// negative time, nothing that is not a number): then the first sum above a query may be found by bisection.
// (store: false in the lanes of a wavefront that only need the answer)
MRS_TG_HD inline bool running_sums(const double* T, int S, double* A, bool store = true) {
  MRS_TG_NO_CONTRACT
  double acc = 0.0;
  bool sorted = true;
  for (int i = 0; i < S; ++i) {
    const double next = acc + T[i];
    sorted = sorted && (next >= acc);
    if (store) A[i] = next;
    acc = next;
  }
  return sorted;
}

struct Located {
  int seg;     // index within the path, -1 = out of range
  double tau;  // seconds from the start of that segment
};

// The first i with A[i] > t: the loop as written when the sums may decrease, a bisection over them when they do not (the
// same index: "A[i] > t" is then false up to it and true from it on).
MRS_TG_HD inline Located locate(const double* T, const double* A, int S, bool sorted, double t) {
  MRS_TG_NO_CONTRACT
  Located r;
  r.seg = -1;
  r.tau = 0.0;
  if (S < 1) return r;
  const double total = A[S - 1];
  if (!(t >= 0.0) || !(total == total)) return r;
  int i;
  if (sorted) {
    int lo = 0, hi = S;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (A[mid] > t)
        hi = mid;
      else
        lo = mid + 1;
    }
    i = lo;
  } else {
    for (i = 0; i < S; ++i)
      if (A[i] > t) break;
  }
  if (i == S) {
    if (t > total) return r;
    i = S - 1;
  }
  const double start = A[i] - T[i];
  r.seg = i;
  r.tau = t - start;
  return r;
}

// p^(O)(tau) of the polynomial c[0 .. 10): Horner over j!/(j-O)! c_j, as sample_path_walk evaluates
template <int O>
MRS_TG_HD inline double derivative(const double* c, double tau) {
  MRS_TG_NO_CONTRACT
  double acc = falling_factorial(kN - 1, O) * c[kN - 1];
  MRS_TG_UNROLL
  for (int j = kN - 2; j >= O; --j) acc = fma(acc, tau, falling_factorial(j, O) * c[j]);
  return acc;
}

// one state row [NO][4] from the segment's coefficients c[4][10]
template <int NO>
MRS_TG_HD inline void state_row(const double* c, double tau, double (&out)[NO][kD]) {
  MRS_TG_UNROLL
  for (int dd = 0; dd < kD; ++dd) {
    const double* cd = c + dd * kN;
    out[0][dd] = derivative<0>(cd, tau);
    if constexpr (NO == kMaxOrders) {
      out[1][dd] = derivative<1>(cd, tau);
      out[2][dd] = derivative<2>(cd, tau);
      out[3][dd] = derivative<3>(cd, tau);
      out[4][dd] = derivative<4>(cd, tau);
    }
  }
  out[0][kD - 1] = wrap_heading(out[0][kD - 1]);
}

// One query's terms of dL/dc of its segment: terms[dim * 10 + j] from its upstream row G[NO][4]
template <int NO>
MRS_TG_HD inline void coeff_terms(const double* G, double tau, double (&terms)[kCoeffElems]) {
  MRS_TG_UNROLL
  for (int dd = 0; dd < kD; ++dd) {
    double g[NO];
    MRS_TG_UNROLL
    for (int o = 0; o < NO; ++o) g[o] = G[o * kD + dd];
    MRS_TG_UNROLL
    for (int j = 0; j < kN; ++j) {
      double w[kN];
      sampvjp::coeff_weights(j, w);
      terms[dd * kN + j] = sampvjp::coeff_term<NO>(j, w, g, tau);
    }
  }
}

// g_q = sum over (o, dim), in the order o * 4 + dim, of G[o][dim] p_dim^(o+1)(tau); c = the segment's coefficients [4][10]
template <int NO>
MRS_TG_HD inline double time_gradient(const double* c, const double* G, double tau) {
  double s = 0.0;
  MRS_TG_UNROLL
  for (int o = 0; o < NO; ++o) {
    double w[kN];
    sampvjp::time_weights(o, w);
    MRS_TG_UNROLL
    for (int dd = 0; dd < kD; ++dd) {
      const double term = sampvjp::time_term(o, w, c + dd * kN, G[o * kD + dd], tau);
      s = (o == 0 && dd == 0) ? term : sampvjp::accumulate(s, term);
    }
  }
  return s;
}

}  // namespace evalq
}  // namespace mrs_tg

// mrs_tg_sample_vjp.hpp -- one sample's share of the backward pass of the sampler (mrs_tg_plan_sample_states_vjp,
// sample_vjp_kernel).  Sample k of a path sits in segment i_k at the time t_k in that segment and is
//   state[k][o][dim] = sum_{j >= o} j!/(j-o)! c[i_k][dim][j] t_k^(j-o),   o = 0 .. n_orders - 1
// (the heading of order 0 wrapped, derivative 1).  With the upstream G[k][o][dim] = dL/dstate[k][o][dim]:
//   dL/dc[i][dim][j] = sum over the samples of segment i, in increasing k, of coeff_term:
//                      sum_{o <= min(j, n_orders-1)} G[k][o][dim] j!/(j-o)! t_k^(j-o)
//   dL/dt_k          = sum over (o, dim) of time_term: G[k][o][dim] p_dim^(o+1)(t_k)
//   dL/dT_i          = -(s_{i+1} + (s_{i+2} + ( ... + s_{S-1}))), s_i = the (o, dim) partials of segment i -- each the sum of
//                      its time_terms in increasing k -- added in the order o * 4 + dim
// Every output element is one accumulator: no sum depends on how the walk chunked the samples.
// Plain double, __host__ __device__ (tests/host/sample_vjp_harness.cpp runs it on the CPU): every product that could fuse is
// an explicit fma or kept apart by contraction being off, so the CPU and the GPU execute the same operations.  The loops are
// written with constant bounds and a predicate, so that the device keeps g[] and w[] in registers.
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace sampvjp {

using mrs_tg::accumulate;
using mrs_tg::kD;
using mrs_tg::kMaxOrders;
using mrs_tg::kN;
constexpr int kCoeffElems = kD * kN;  // (dim, j) = (e / kN, e % kN)

// the weights an output element multiplies with, formed once: w[o] = j!/(j-o)! for the coefficient element j (o <= 4 used),
// w[j] = j!/(j-o-1)! for the time element of order o
MRS_TG_HD inline void coeff_weights(int j, double (&w)[kN]) {
  MRS_TG_UNROLL
  for (int o = 0; o < kN; ++o) w[o] = falling_factorial_predicated(j, o);
}
MRS_TG_HD inline void time_weights(int o, double (&w)[kN]) {
  MRS_TG_UNROLL
  for (int j = 0; j < kN; ++j) w[j] = falling_factorial_predicated(j, o + 1);
}

// One sample's term of dL/dc[dim][j]: g[o] = G[k][o][dim], w = coeff_weights(j).  With omax = min(j, NO-1):
// t^(j-omax) sum_{o <= omax} g[o] w[o] t^(omax-o) -- Horner over the orders o = 0 .. omax, then the power by repeated
// multiplication.
template <int NO>
MRS_TG_HD inline double coeff_term(int j, const double (&w)[kN], const double (&g)[NO], double t) {
  MRS_TG_NO_CONTRACT
  const int omax = j < NO - 1 ? j : NO - 1;
  double acc = g[0] * w[0];
  MRS_TG_UNROLL
  for (int o = 1; o < NO; ++o)
    if (o <= omax) acc = fma(acc, t, g[o] * w[o]);
  MRS_TG_UNROLL
  for (int n = 0; n < kN - 1; ++n)
    if (n < j - omax) acc = acc * t;
  return acc;
}

// One sample's term of the (o, dim) time partial: g = G[k][o][dim], c = the kN coefficients of dim in the sample's segment,
// w = time_weights(o): g p_dim^(o+1)(t), Horner from j = 9 down to o + 1
MRS_TG_HD inline double time_term(int o, const double (&w)[kN], const double* c, double g, double t) {
  MRS_TG_NO_CONTRACT
  double acc = w[kN - 1] * c[kN - 1];
  MRS_TG_UNROLL
  for (int j = kN - 2; j >= 1; --j)
    if (j >= o + 1) acc = fma(acc, t, w[j] * c[j]);
  return g * acc;
}

// dL/dT from the segments' sums s[0 .. S): out[i] = -(s[i+1] + (s[i+2] + ...)), from the last segment downwards
MRS_TG_HD inline void time_gradients(const double* s, int S, double* out) {
  MRS_TG_NO_CONTRACT
  double r = 0.0;
  for (int i = S - 1; i >= 0; --i) {
    out[i] = 0.0 - r;
    r = s[i] + r;
  }
}

}  // namespace sampvjp
}  // namespace mrs_tg

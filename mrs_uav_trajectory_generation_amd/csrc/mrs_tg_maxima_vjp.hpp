// mrs_tg_maxima_vjp.hpp -- one entry's share of the backward pass of the segment maxima (mrs_tg_plan_segment_maxima_vjp,
// segment_maxima_vjp_kernel).  An entry (k, group) of a segment with physical-time coefficients
// c[dim][j] and time T has the value M = max over t in [0, T] of |p^(k)(t)|, p^(k) the group's k-th derivatives.  With t* the
// maximiser and u = p^(k)(t*) / |p^(k)(t*)|, by the envelope theorem:
//   dM/dc[dim][j] = u_dim j!/(j-k)! t*^(j-k)   (j >= k, dim in the group; 0 elsewhere)
//   dM/dT         = u . p^(k+1)(T) if t* = T, else 0
// The seed abscissa is the forward search's winner (max_mag2_search<1, true>, mrs_tg_maxima.hpp): the value is accurate there
// but the abscissa only to ~3e-7 of the segment, so an interior seed is refined by at most kRefineSteps Newton steps on
// g = 1/2 dm2/dtau (stop when |dtau| <= 2^-50); the refined abscissa is kept only if it lies in the seed's grid cell, g' < 0
// there and m2 did not fall (by more than its evaluation's rounding, kEps) -- otherwise the gradient is taken at the seed.  End-point
// seeds (tau = 0 or 1) are not refined.
// A zero maximum and an entry with a zero upstream contribute exactly 0.
// Plain double, __host__ __device__ (tests/host/maxima_vjp_harness.cpp runs it on the CPU): every product that could fuse is an
// explicit fma or kept apart by contraction being off, so the CPU and the GPU execute the same operations.
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace maxvjp {

using mrs_tg::kD;
using mrs_tg::kN;
constexpr int kEntries = 9;
constexpr int kRefineSteps = 4;
constexpr double kRefineStop = 0x1p-50;
// the refinement polishes the forward's own maximiser, it does not look for another: a seed the polish left at its stopping
// accuracy (3e-7) moves less than this; a winning grid point beside a peak the grid did not bracket would move further, and
// keeps its own gradient (that of the value the forward returned)
constexpr double kRefineReach = 0x1p-20;
// "m2 did not fall": a seed the forward's polish left within ~1e-8 of the maximiser sits where m2 is flat to below the rounding
// of its own evaluation (Horner with cancelling terms), so the refined m2 may come out lower although the abscissa improved.
// A fall counts only beyond that rounding: 2 (2 N0 + 2) eps sum_q A_q^2, A_q = sum_j |d0_qj| tau^j (the evaluation's bound).
constexpr double kEps = 0x1p-53;

// group 0 = {x, y} (dimensions 0, 1), 1 = {z} (2), 2 = {heading} (3)
MRS_TG_HD constexpr int group_of_dim(int dim) { return dim < 2 ? 0 : dim - 1; }

// What one entry leaves for the segment's sums: t* in seconds, s = G u (the group's components; s[1] = 0 for a 1-D group)
// and the entry's time gradient G dM/dT.
struct EntryTerms {
  double t, s0, s1, dT;
};

// q^(K) (derivative K in normalised time tau = t / T) of the NDIM dimensions of a group, coefficients formed as the forward
// forms them (c_j T^j, then j!/(j-K)! of the shifted index)
template <int K, int NDIM>
struct QPoly {
  static constexpr int N0 = kN - K;
  double d0[NDIM][N0];

  MRS_TG_HD void init(const double* c, int dim0, double T) {
    MRS_TG_NO_CONTRACT
    double cb[NDIM][kN];
    double tp = 1.0;
    MRS_TG_UNROLL
    for (int j = 0; j < kN; ++j) {
      MRS_TG_UNROLL
      for (int q = 0; q < NDIM; ++q) cb[q][j] = c[(dim0 + q) * kN + j] * tp;
      tp *= T;
    }
    MRS_TG_UNROLL
    for (int q = 0; q < NDIM; ++q)
      MRS_TG_UNROLL
      for (int j = 0; j < N0; ++j) d0[q][j] = cb[q][j + K] * falling_factorial(j + K, K);
  }

  // the rounding bound of m2 at tau (see kEps)
  MRS_TG_HD double m2_rounding(double tau) const {
    MRS_TG_NO_CONTRACT
    double s = 0.0;
    MRS_TG_UNROLL
    for (int q = 0; q < NDIM; ++q) {
      double a = fabs(d0[q][N0 - 1]);
      MRS_TG_UNROLL
      for (int j = N0 - 2; j >= 0; --j) a = fma(a, tau, fabs(d0[q][j]));
      s = fma(a, a, s);
    }
    return (2.0 * (2 * N0 + 2)) * kEps * s;
  }

  // v0 = q^(K)(tau), v1 = q^(K+1)(tau), h2 = q^(K+2)(tau) / 2 per dimension (one nested Horner pass);
  // m2 = sum v0^2, g = sum v0 v1 = dm2/dtau / 2, dg = dg/dtau
  MRS_TG_HD void eval(double tau, double (&v0)[NDIM], double (&v1)[NDIM], double& m2, double& g, double& dg) const {
    MRS_TG_NO_CONTRACT
    m2 = 0.0;
    g = 0.0;
    dg = 0.0;
    MRS_TG_UNROLL
    for (int q = 0; q < NDIM; ++q) {
      double a0 = d0[q][N0 - 1], a1 = 0.0, h2 = 0.0;
      MRS_TG_UNROLL
      for (int j = N0 - 2; j >= 0; --j) {
        h2 = fma(h2, tau, a1);
        a1 = fma(a1, tau, a0);
        a0 = fma(a0, tau, d0[q][j]);
      }
      v0[q] = a0;
      v1[q] = a1;
      m2 = fma(a0, a0, m2);
      g = fma(a0, a1, g);
      dg = dg + fma(a1, a1, 2.0 * (a0 * h2));
    }
  }
};

// The refined abscissa of a seed (see the file comment); [lo, hi] is the seed's grid cell
template <int K, int NDIM>
MRS_TG_HD double refine_tau(const QPoly<K, NDIM>& qp, double tau, double lo, double hi) {
  MRS_TG_NO_CONTRACT
  if (!(tau > 0.0 && tau < 1.0)) return tau;
  double v0[NDIM], v1[NDIM], m2_seed, g, dg;
  qp.eval(tau, v0, v1, m2_seed, g, dg);
  double t = tau, m2 = m2_seed;
  for (int it = 0; it < kRefineSteps; ++it) {
    const double step = -g / dg;
    t = t + step;
    qp.eval(t, v0, v1, m2, g, dg);  // (m2, dg at the final t: the acceptance test below)
    if (!(fabs(step) > kRefineStop)) break;
  }
  return (t >= lo && t <= hi && fabs(t - tau) <= kRefineReach && dg < 0.0 && m2 >= m2_seed - qp.m2_rounding(tau)) ? t : tau;
}

template <int K, int NDIM>
MRS_TG_HD EntryTerms entry_terms_k(const double* c, double T, int dim0, double tau_seed, double lo, double hi, double G) {
  MRS_TG_NO_CONTRACT
  QPoly<K, NDIM> qp;
  qp.init(c, dim0, T);
  const double tau = refine_tau(qp, tau_seed, lo, hi);
  EntryTerms e{tau * T, 0.0, 0.0, 0.0};
  if (G == 0.0) return e;  // exactly 0, whatever the maximum is
  double v0[NDIM], v1[NDIM], m2, g, dg;
  qp.eval(tau, v0, v1, m2, g, dg);
  if (!(m2 > 0.0)) return e;  // a zero maximum: the entry contributes 0 (no direction to take)
  const double inv = 1.0 / sqrt(m2);
  double u[NDIM];
  MRS_TG_UNROLL
  for (int q = 0; q < NDIM; ++q) u[q] = v0[q] * inv;
  e.s0 = G * u[0];
  e.s1 = (NDIM == 2) ? G * u[NDIM - 1] : 0.0;
  if (tau == 1.0) {  // the maximum sits at the segment's end: dM/dT = u . p^(k+1)(T) = u . q^(k+1)(1) / T^(k+1)
    const double ti = 1.0 / T;
    double sc = ti;
    MRS_TG_UNROLL
    for (int n = 0; n < K; ++n) sc = sc * ti;
    double d = 0.0;
    MRS_TG_UNROLL
    for (int q = 0; q < NDIM; ++q) d = fma(u[q], v1[q], d);
    e.dT = G * (d * sc);
  }
  return e;
}

// The inputs an entry reads are usable: 0 < T < inf and the group's coefficients finite (a segment whose nine entries are not
// all usable gets zero rows)
MRS_TG_HD inline bool entry_valid(const double* c, double T, int which) {
  const int grp = which % 3, dim0 = grp == 0 ? 0 : grp + 1, nd = grp == 0 ? 2 : 1;
  bool ok = T > 0.0 && T < INFINITY;
  for (int i = 0; i < nd * kN; ++i) ok = ok && fabs(c[dim0 * kN + i]) < INFINITY;
  return ok;
}

// One entry (which = 3 (k-1) + group) of a valid segment, seeded at the forward's winner tau_seed in its cell [lo, hi], with
// upstream G = dL/dM
MRS_TG_HD inline EntryTerms entry_terms(const double* c, double T, int which, double tau_seed, double lo, double hi, double G) {
  const int k = which / 3 + 1, grp = which % 3;
  if (grp == 0) {
    return (k == 1)   ? entry_terms_k<1, 2>(c, T, 0, tau_seed, lo, hi, G)
           : (k == 2) ? entry_terms_k<2, 2>(c, T, 0, tau_seed, lo, hi, G)
                      : entry_terms_k<3, 2>(c, T, 0, tau_seed, lo, hi, G);
  }
  const int dim = grp + 1;
  return (k == 1)   ? entry_terms_k<1, 1>(c, T, dim, tau_seed, lo, hi, G)
         : (k == 2) ? entry_terms_k<2, 1>(c, T, dim, tau_seed, lo, hi, G)
                    : entry_terms_k<3, 1>(c, T, dim, tau_seed, lo, hi, G);
}

// The segment's sums, entry w of the segment at e[w * stride]: dL/dc[dim][j] = sum over k = 1, 2, 3 (in that order) of
// s_dim j!/(j-k)! t*_k^(j-k) of the entry (k, group of dim)
MRS_TG_HD inline double coeff_gradient(const EntryTerms* e, int stride, int dim, int j) {
  MRS_TG_NO_CONTRACT
  const int grp = group_of_dim(dim);
  double acc = 0.0;
  for (int k = 1; k <= 3; ++k) {
    if (j < k) break;
    const EntryTerms& x = e[(3 * (k - 1) + grp) * stride];
    const double s = (dim == 1) ? x.s1 : x.s0;
    if (s == 0.0) continue;
    double p = 1.0;
    for (int n = 0; n < j - k; ++n) p = p * x.t;
    acc = acc + (s * falling_factorial(j, k)) * p;
  }
  return acc;
}

// dL/dT = the nine entries' time terms, summed in entry order
MRS_TG_HD inline double time_gradient(const EntryTerms* e, int stride) {
  MRS_TG_NO_CONTRACT
  double acc = 0.0;
  for (int w = 0; w < kEntries; ++w) acc = acc + e[w * stride].dT;
  return acc;
}

}  // namespace maxvjp
}  // namespace mrs_tg

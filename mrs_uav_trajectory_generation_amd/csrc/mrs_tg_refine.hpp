// mrs_tg_refine.hpp -- one lane's share of the refinement pass (MRS_TG_FLAG_REFINE): iterative refinement of a solved path's
// linear QP with a double-double residual, one lane = one (path, dimension), any fixed / free pattern (5 x 5 vertex blocks).
//
// The solve kernels return coefficients c that are accurate to cond(R_pp) * eps relative; R_pp's condition number grows like
// (T_max / T_min)^7 between neighbouring segments, so a 0.18 s segment between 4-5 s ones leaves 1e-8.  Here:
//   1. the vertex derivatives d are taken from the coefficients (d_k = k! c_k at a segment start -- two_prod, exact; the free
//      slots of the last vertex from the last segment at T, in double-double) and held in double-double;
//   2. the residual r = R_pf d_f + R_pp d_p of the free slots is formed in double-double, segment by segment, from
//      H(T) = T^(1-2d) D_T Hbar D_T with the double-double tables of mrs_tg_constants_dd.h;
//   3. R_pp delta = -r is solved in double by a block-tridiagonal Cholesky (the elimination of mrs_tg_general.hpp: masked
//      5 x 5 vertex blocks, a vanishing pivot leaves its variable at zero), factored once, solved for every step;
//   4. d_p += delta in double-double, kept only if the residual norm (each free row scaled by 1 / its diagonal entry of R_pp,
//      per dimension) went down -- else the previous iterate stays and the lane stops; at most kRefineSteps steps;
//   5. c = A^-1(T) d per segment in double-double (c_k = cbar_k / T^k, cbar = Abar^-1 D_T d), rounded once; the lane's share
//      of the cost 0.5 sum d^T H(T) d in double-double.
// The code is __host__ __device__ over plain arrays (tests/host/refine_harness.cpp runs it on the CPU against the fixtures).
// Error-free transformations need every product rounded on its own: contraction is switched off inside the helpers and the
// fused steps are explicit fma.
#pragma once

#include "mrs_tg_constants.h"
#include "mrs_tg_constants_dd.h"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace refine {

constexpr int kTri = kB * (kB + 1) / 2;
constexpr int kRefineSteps = 3;
// per vertex and lane: L (diagonal entries hold 1 / L_cc), W, z, two double-double iterates (hi[5], lo[5] each)
constexpr int kWsL = 0, kWsW = kTri, kWsZ = kWsW + kB * kB, kWsD = kWsZ + kB, kWsPerVertex = kWsD + 4 * kB;

#if defined(__HIP_DEVICE_COMPILE__)
static __constant__ double c_rf_abar_inv[kN][kN][2] = MRS_TG_ABAR_INV_DD_INIT;
static __constant__ double c_rf_hbar[kB][kN][kN][2] = MRS_TG_HBAR_DD_INIT;
#define MRS_TG_RF_ABAR c_rf_abar_inv
#define MRS_TG_RF_HBAR c_rf_hbar
#else
static const double h_rf_abar_inv[kN][kN][2] = MRS_TG_ABAR_INV_DD_INIT;
static const double h_rf_hbar[kB][kN][kN][2] = MRS_TG_HBAR_DD_INIT;
#define MRS_TG_RF_ABAR h_rf_abar_inv
#define MRS_TG_RF_HBAR h_rf_hbar
#endif

// ---- double-double arithmetic (Dekker / Knuth error-free transformations) -----------------------------------------------
struct dd {
  double hi, lo;
};

MRS_TG_HD inline dd two_sum(double a, double b) {
  MRS_TG_NO_CONTRACT
  const double s = a + b;
  const double bb = s - a;
  return dd{s, (a - (s - bb)) + (b - bb)};
}
MRS_TG_HD inline dd quick_two_sum(double a, double b) {
  MRS_TG_NO_CONTRACT
  const double s = a + b;
  return dd{s, b - (s - a)};
}
MRS_TG_HD inline dd two_prod(double a, double b) {
  MRS_TG_NO_CONTRACT
  const double p = a * b;
  return dd{p, fma(a, b, -p)};
}
MRS_TG_HD inline dd dd_add(dd x, dd y) {
  MRS_TG_NO_CONTRACT
  dd s = two_sum(x.hi, y.hi);
  const dd t = two_sum(x.lo, y.lo);
  s.lo += t.hi;
  s = quick_two_sum(s.hi, s.lo);
  s.lo += t.lo;
  return quick_two_sum(s.hi, s.lo);
}
MRS_TG_HD inline dd dd_neg(dd x) { return dd{-x.hi, -x.lo}; }
MRS_TG_HD inline dd dd_mul(dd x, dd y) {
  MRS_TG_NO_CONTRACT
  dd p = two_prod(x.hi, y.hi);
  p.lo = fma(x.hi, y.lo, fma(x.lo, y.hi, p.lo));
  return quick_two_sum(p.hi, p.lo);
}
MRS_TG_HD inline dd dd_mul_d(dd x, double b) {
  MRS_TG_NO_CONTRACT
  dd p = two_prod(x.hi, b);
  p.lo = fma(x.lo, b, p.lo);
  return quick_two_sum(p.hi, p.lo);
}
MRS_TG_HD inline dd dd_div(dd x, dd y) {
  MRS_TG_NO_CONTRACT
  const double q1 = x.hi / y.hi;
  dd r = dd_add(x, dd_neg(dd_mul_d(y, q1)));
  const double q2 = r.hi / y.hi;
  r = dd_add(r, dd_neg(dd_mul_d(y, q2)));
  const double q3 = r.hi / y.hi;
  return dd_add(quick_two_sum(q1, q2), dd{q3, 0.0});
}
// acc += a * x with a a double-double table entry { hi, lo }: the low-order products and the rounding errors of the sum are
// gathered in acc.lo in double (relative error of the sum ~ n eps^2)
MRS_TG_HD inline void dd_fma_acc(dd& acc, const double (&a)[2], dd x) {
  MRS_TG_NO_CONTRACT
  const dd p = two_prod(a[0], x.hi);
  const dd s = two_sum(acc.hi, p.hi);
  acc.hi = s.hi;
  acc.lo = acc.lo + (s.lo + fma(a[0], x.lo, fma(a[1], x.hi, p.lo)));
}
MRS_TG_HD inline dd dd_norm(dd x) { return quick_two_sum(x.hi, x.lo); }

// 1 / sqrt of a Cholesky pivot, the device's way: NOT the correctly rounded one of the solve's backward pass
// (vjp::inv_sqrt_pivot_exact) -- the correction solve only has to contract, the residual is what is exact
MRS_TG_HD inline double inv_sqrt_pivot_rsq(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  // v_rsq_f64 + one third-order step (rsqrt_refined of mrs_tg_device.hpp); a pivot <= 0 is rejected (variable left at 0)
  const double y = __builtin_amdgcn_rsq(x);
  const double e = fma(-(x * y), y, 1.0);
  const double r = fma(y * e, fma(e, 0.375, 0.5), y);
  return (x > 0.0) ? r : 0.0;
#else
  return (x > 0.0) ? 1.0 / std::sqrt(x) : 0.0;
#endif
}

using LaneWs = LaneWsT<kWsPerVertex>;

// T^0..T^4 and T^(1-2d) * T^0..4 in double-double
struct SegPowers {
  dd tp[kB];
  dd sp[kB];
};
MRS_TG_HD inline void seg_powers(double T, int d, SegPowers& P) {
  P.tp[0] = dd{1.0, 0.0};
  P.tp[1] = dd{T, 0.0};
  MRS_TG_UNROLL
  for (int k = 2; k < kB; ++k) P.tp[k] = dd_mul_d(P.tp[k - 1], T);
  dd t2dm1 = dd{1.0, 0.0};  // T^(2d - 1), d >= 1; d = 0: T^(1-0) = T
  for (int k = 0; k < 2 * d - 1; ++k) t2dm1 = dd_mul_d(t2dm1, T);
  const dd s = (d == 0) ? dd{T, 0.0} : dd_div(dd{1.0, 0.0}, t2dm1);
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) P.sp[k] = dd_mul(s, P.tp[k]);
}

MRS_TG_HD inline double slot_value(const double* vals, int v, int k, int dim) { return vals[((size_t)v * kB + k) * kD + dim]; }

MRS_TG_HD inline void load_iterate(const LaneWs& w, int v, int buf, dd (&x)[kB]) {
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) x[k] = dd{w.at(v, kWsD + buf * 2 * kB + k), w.at(v, kWsD + buf * 2 * kB + kB + k)};
}
MRS_TG_HD inline void store_iterate(const LaneWs& w, int v, int buf, const dd (&x)[kB]) {
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) {
    w.at(v, kWsD + buf * 2 * kB + k) = x[k].hi;
    w.at(v, kWsD + buf * 2 * kB + kB + k) = x[k].lo;
  }
}

// gbar = Hbar_d dbar, dbar = D_T [ds; de]: the segment's Hessian product in unit time (the caller scales row a by sp[a % 5])
MRS_TG_HD inline void segment_hessian_product(int d, const SegPowers& P, const dd (&ds)[kB], const dd (&de)[kB], dd (&dbar)[kN],
                                              dd (&gbar)[kN]) {
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) {
    dbar[k] = dd_mul(P.tp[k], ds[k]);
    dbar[kB + k] = dd_mul(P.tp[k], de[k]);
  }
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) {
    dd acc{0.0, 0.0};
    MRS_TG_UNROLL
    for (int b = 0; b < kN; ++b) dd_fma_acc(acc, MRS_TG_RF_HBAR[d][a][b], dbar[b]);
    gbar[a] = dd_norm(acc);
  }
}

// Block-tridiagonal Cholesky of R_pp (double, from the double tables), factors to the workspace: per vertex L (1 / L_cc on the
// diagonal) and W = L^-1 E.  The masking and the pivot rule are those of gen_factor (mrs_tg_general.hpp).
MRS_TG_HD inline void factor_lane(const uint8_t* mask, int v0, int S, int d, const double* times, const LaneWs& w) {
  double Sm[kTri];
  MRS_TG_UNROLL
  for (int e = 0; e < kTri; ++e) Sm[e] = 0.0;
  for (int v = 0; v <= S; ++v) {
    unsigned fs = 0u, fe = 0u;
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      if (slot_free(mask, v0 + v, k)) fs |= 1u << k;
      if (v < S && slot_free(mask, v0 + v + 1, k)) fe |= 1u << k;
    }
    double p2[9];  // H(a, b) = Hbar[a][b] T^(1 - 2d + a % 5 + b % 5)
    const double T = times[v < S ? v : S - 1];
    double td = 1.0;
    for (int k = 0; k < d; ++k) td *= T;
    p2[0] = T / (td * td);
    MRS_TG_UNROLL
    for (int m = 1; m < 9; ++m) p2[m] = p2[m - 1] * T;
    auto H = [&](int a, int b) { return MRS_TG_RF_HBAR[d][a][b][0] * p2[(a % kB) + (b % kB)]; };
    if (v < S) {
      MRS_TG_UNROLL
      for (int r = 0; r < kB; ++r)
        MRS_TG_UNROLL
        for (int c = 0; c <= r; ++c) Sm[tri5(r, c)] += H(r, c);
    }
    // mask, factor
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r) {
      const bool fr = (fs >> r) & 1u;
      MRS_TG_UNROLL
      for (int c = 0; c <= r; ++c) {
        const bool fc = (fs >> c) & 1u;
        const double x = Sm[tri5(r, c)];
        Sm[tri5(r, c)] = (r == c) ? (fr ? x : 1.0) : ((fr && fc) ? x : 0.0);
      }
    }
    double L[kTri], Linv[kB];
    MRS_TG_UNROLL
    for (int c = 0; c < kB; ++c) {
      double dsum = Sm[tri5(c, c)];
      MRS_TG_UNROLL
      for (int m = 0; m < c; ++m) dsum = fma(-L[tri5(c, m)], L[tri5(c, m)], dsum);
      const double inv = inv_sqrt_pivot_rsq(dsum);
      L[tri5(c, c)] = fmax(dsum * inv, 1.0e-300);
      Linv[c] = inv;
      MRS_TG_UNROLL
      for (int r = c + 1; r < kB; ++r) {
        double s = Sm[tri5(r, c)];
        MRS_TG_UNROLL
        for (int m = 0; m < c; ++m) s = fma(-L[tri5(r, m)], L[tri5(c, m)], s);
        L[tri5(r, c)] = s * inv;
      }
    }
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r)
      MRS_TG_UNROLL
      for (int c = 0; c <= r; ++c) w.at(v, kWsL + tri5(r, c)) = (r == c) ? Linv[r] : L[tri5(r, c)];
    if (v == S) {  // the last vertex couples to nothing: its W block is zero, written so that no sweep reads undefined memory
      MRS_TG_UNROLL
      for (int e = 0; e < kB * kB; ++e) w.at(v, kWsW + e) = 0.0;
      break;
    }
    double W[kB][kB];
    MRS_TG_UNROLL
    for (int c = 0; c < kB; ++c)
      MRS_TG_UNROLL
      for (int r = 0; r < kB; ++r) {
        const bool on = ((fs >> r) & 1u) && ((fe >> c) & 1u);
        double s = on ? H(r, kB + c) : 0.0;
        MRS_TG_UNROLL
        for (int m = 0; m < r; ++m) s = fma(-L[tri5(r, m)], W[m][c], s);
        W[r][c] = s * Linv[r];
      }
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r)
      MRS_TG_UNROLL
      for (int c = 0; c < kB; ++c) w.at(v, kWsW + r * kB + c) = W[r][c];
    // Schur complement on the next vertex
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r)
      MRS_TG_UNROLL
      for (int c = 0; c <= r; ++c) {
        double s = H(kB + r, kB + c);
        MRS_TG_UNROLL
        for (int m = 0; m < kB; ++m) s = fma(-W[m][r], W[m][c], s);
        Sm[tri5(r, c)] = s;
      }
  }
}

// Residual of iterate `buf` in double-double, segment by segment, and in the same sweep the forward substitution
// z = L^-1 (-r) of the correction solve (z to the workspace).  Returns sum over free rows of r^2 / R_aa.
// The loads a vertex needs (its factors, the iterate two vertices ahead) are issued before the segment's double-double
// arithmetic, so that their latency hides behind it: one lane's sweep is a chain over the vertices.
MRS_TG_HD inline void load_factors(const LaneWs& w, int v, double (&L)[kTri], double (&W)[kB * kB]) {
  MRS_TG_UNROLL
  for (int e = 0; e < kTri; ++e) L[e] = w.at(v, kWsL + e);
  MRS_TG_UNROLL
  for (int e = 0; e < kB * kB; ++e) W[e] = w.at(v, kWsW + e);
}

MRS_TG_HD inline double residual_forward(const uint8_t* mask, int v0, int S, int d, const double* times, const LaneWs& w, int buf) {
  double norm = 0.0;
  dd carry[kB];
  double carry_diag[kB], zprev[kB];
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) {
    carry[k] = dd{0.0, 0.0};
    carry_diag[k] = 0.0;
    zprev[k] = 0.0;
  }
  dd ds[kB], de[kB], dn[kB];
  load_iterate(w, 0, buf, ds);
  load_iterate(w, S < 1 ? S : 1, buf, de);
  for (int v = 0; v <= S; ++v) {
    // this vertex's factors, the previous vertex's coupling block, the free slots, the iterate at v + 2
    double L[kTri], Wp[kB * kB];
    MRS_TG_UNROLL
    for (int e = 0; e < kTri; ++e) L[e] = w.at(v, kWsL + e);
    MRS_TG_UNROLL
    for (int e = 0; e < kB * kB; ++e) Wp[e] = w.at(v > 0 ? v - 1 : 0, kWsW + e);  // (v = 0: any finite block, zprev = 0)
    const unsigned fb = free_bits(mask, v0 + v);
    const double T = times[v < S ? v : S - 1];
    load_iterate(w, v + 2 <= S ? v + 2 : S, buf, dn);
    dd r[kB];
    double diag[kB];
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      r[k] = carry[k];
      diag[k] = carry_diag[k];
    }
    if (v < S) {
      SegPowers P;
      seg_powers(T, d, P);
      dd dbar[kN], gbar[kN];
      segment_hessian_product(d, P, ds, de, dbar, gbar);
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) {
        r[k] = dd_add(r[k], dd_mul(P.sp[k], gbar[k]));
        carry[k] = dd_mul(P.sp[k], gbar[kB + k]);
        const double tk = P.tp[k].hi;
        diag[k] += MRS_TG_RF_HBAR[d][k][k][0] * P.sp[0].hi * tk * tk;
        carry_diag[k] = MRS_TG_RF_HBAR[d][kB + k][kB + k][0] * P.sp[0].hi * tk * tk;
      }
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      ds[k] = de[k];
      de[k] = dn[k];
    }
    // forward substitution on vertex v: y = -r - W_{v-1}^T z_{v-1}, z = L^-1 y (constrained rows: 0; at v = 0 zprev is 0)
    double y[kB];
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      const bool fr = (fb >> k) & 1u;
      const double rk = r[k].hi + r[k].lo;
      if (fr && diag[k] > 0.0) norm += rk * rk / diag[k];
      double s = -rk;
      MRS_TG_UNROLL
      for (int m = 0; m < kB; ++m) s = fma(-Wp[m * kB + k], zprev[m], s);
      y[k] = fr ? s : 0.0;
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      double s = y[k];
      MRS_TG_UNROLL
      for (int m = 0; m < k; ++m) s = fma(-L[tri5(k, m)], zprev[m], s);
      zprev[k] = s * L[tri5(k, k)];  // (zprev[m < k] already holds this vertex's z)
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) w.at(v, kWsZ + k) = zprev[k];
  }
  return norm;
}

// Back substitution x = L^-T (z - W x_next) from the last vertex down; iterate `dst` = iterate `src` + x on the free slots.
// Everything a vertex needs is loaded in one round before its arithmetic.
MRS_TG_HD inline void backward_update(const uint8_t* mask, int v0, int S, const LaneWs& w, int src, int dst) {
  double xn[kB];
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) xn[k] = 0.0;  // (the last vertex has no successor: W x_next = 0)
  for (int v = S; v >= 0; --v) {
    double L[kTri], W[kB * kB], z[kB];
    load_factors(w, v, L, W);
    if (v == S) {  // (no successor: W x_next = 0 whatever the block holds)
      MRS_TG_UNROLL
      for (int e = 0; e < kB * kB; ++e) W[e] = 0.0;
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) z[k] = w.at(v, kWsZ + k);
    dd cur[kB];
    load_iterate(w, v, src, cur);
    const unsigned fb = free_bits(mask, v0 + v);
    double t[kB], x[kB];
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r) {
      double s = z[r];
      MRS_TG_UNROLL
      for (int c = 0; c < kB; ++c) s = fma(-W[r * kB + c], xn[c], s);
      t[r] = s;
    }
    MRS_TG_UNROLL
    for (int r = kB - 1; r >= 0; --r) {
      double s = t[r];
      MRS_TG_UNROLL
      for (int m = r + 1; m < kB; ++m) s = fma(-L[tri5(m, r)], x[m], s);
      x[r] = s * L[tri5(r, r)];
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      const bool fr = (fb >> k) & 1u;
      x[k] = fr ? x[k] : 0.0;
      if (fr) cur[k] = dd_add(cur[k], dd{x[k], 0.0});
      xn[k] = x[k];
    }
    store_iterate(w, v, dst, cur);
  }
}

// The whole pass for one lane.  coeffs_path: segment i, this dimension at coeffs_path[(i * kD + dim) * kN + k] (read, then
// rewritten).  cost_out: this dimension's share of 0.5 sum d^T H d in double-double.  Returns the accepted steps and whether
// the guard stopped the lane.
struct RefineOutcome {
  int steps;    // accepted correction steps, 0 .. kRefineSteps
  int refused;  // 1: the lane stopped because a step did not lower the residual (the guard), 0: it ran out of steps or
                // reached a zero residual
};

MRS_TG_HD inline RefineOutcome refine_lane(const uint8_t* mask, const double* vals, int v0, int S, int d, int dim, const double* times,
                                 double* coeffs_path, const LaneWs& w, dd& cost_out) {
  // 1. vertex derivatives in double-double, iterate 0
  constexpr double kFact[kB] = {1.0, 1.0, 2.0, 6.0, 24.0};
  for (int v = 0; v <= S; ++v) {
    dd x[kB];
    const int seg = v < S ? v : S - 1;
    const double* c = coeffs_path + ((size_t)seg * kD + dim) * kN;
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      if (!slot_free(mask, v0 + v, k)) {
        x[k] = dd{slot_value(vals, v0 + v, k, dim), 0.0};
      } else if (v < S) {
        x[k] = two_prod(c[k], kFact[k]);
      } else {  // p^(k)(T) of the last segment, Horner in double-double
        const double T = times[S - 1];
        dd acc{0.0, 0.0};
        MRS_TG_UNROLL
        for (int j = kN - 1; j >= k; --j) {
          double f = 1.0;
          MRS_TG_UNROLL
          for (int m = j - k + 1; m <= j; ++m) f *= (double)m;  // j! / (j - k)!, an exact integer
          acc = dd_add(dd_mul_d(acc, T), two_prod(c[j], f));
        }
        x[k] = acc;
      }
    }
    store_iterate(w, v, 0, x);
  }
  // 2.-4. factor once, then residual / correction steps with the guard
  factor_lane(mask, v0, S, d, times, w);
  int cur = 0, steps = 0, refused = 0;
  double norm = residual_forward(mask, v0, S, d, times, w, cur);
  for (int it = 0; it < kRefineSteps && norm > 0.0; ++it) {
    backward_update(mask, v0, S, w, cur, 1 - cur);
    const double nt = residual_forward(mask, v0, S, d, times, w, 1 - cur);
    if (!(nt < norm)) {  // (NaN included) the step did not help: keep the previous iterate
      refused = 1;
      break;
    }
    cur = 1 - cur;
    norm = nt;
    ++steps;
  }
  // 5. coefficients and cost in double-double
  dd cost{0.0, 0.0};
  dd ds[kB], de[kB];
  dd dn[kB];
  load_iterate(w, 0, cur, ds);
  load_iterate(w, 1, cur, de);
  for (int i = 0; i < S; ++i) {
    load_iterate(w, i + 2 <= S ? i + 2 : S, cur, dn);  // (prefetch: the next segment's end vertex)
    const double T = times[i];
    SegPowers P;
    seg_powers(T, d, P);
    dd dbar[kN], gbar[kN];
    segment_hessian_product(d, P, ds, de, dbar, gbar);
    dd q{0.0, 0.0};
    MRS_TG_UNROLL
    for (int a = 0; a < kN; ++a) q = dd_add(q, dd_mul(dbar[a], gbar[a]));
    cost = dd_add(cost, dd_mul_d(dd_mul(q, P.sp[0]), 0.5));
    const dd invT = dd_div(dd{1.0, 0.0}, dd{T, 0.0});
    dd ip{1.0, 0.0};  // T^-k
    double* c = coeffs_path + ((size_t)i * kD + dim) * kN;
    MRS_TG_UNROLL
    for (int k = 0; k < kN; ++k) {
      dd acc{0.0, 0.0};
      MRS_TG_UNROLL
      for (int j = 0; j < kN; ++j) dd_fma_acc(acc, MRS_TG_RF_ABAR[k][j], dbar[j]);
      const dd ck = dd_mul(dd_norm(acc), ip);
      c[k] = ck.hi + ck.lo;
      ip = dd_mul(ip, invT);
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      ds[k] = de[k];
      de[k] = dn[k];
    }
  }
  cost_out = cost;
  return RefineOutcome{steps, refused};
}

}  // namespace refine
}  // namespace mrs_tg

// mrs_tg_vjp.hpp -- one lane's share of the backward pass of the fixed-times solve (mrs_tg_plan_solve_vjp): the exact chain rule
// of the linear QP at the returned solution, one lane = one (path, dimension), any fixed / free pattern (5 x 5 vertex blocks).
// DESIGN.md section 4c has the derivation; in short, per dimension, with u_i = (d_i, d_{i+1}) the segment's end-point
// derivatives, c_i = A(T_i)^-1 u_i, J = 1/2 sum u_i^T H_i u_i, H(T) = T^(1-2d) D_T Hbar D_T, upstream G_i = dL/dc_i and g = dL/dJ:
//   1. abar_i = A^-T G_i + g H_i u_i, scattered into the vertex slots: a;
//   2. R_pp lambda = a_P by the masked block-tridiagonal Cholesky of mrs_tg_general.hpp (a vanishing pivot leaves its lambda 0);
//   3. dL/dd_F = (a - R lambda~)_F, lambda~ = lambda on the free slots and 0 on the fixed ones; free slots get 0;
//   4. dL/dT_i = G_i . dc_i/dT|_u + g/2 u_i^T H_i' u_i - lambda~_i^T H_i' u_i, H'_ab = (1 - 2d + s(a) + s(b)) H_ab / T,
//      summed over the four dimensions by the caller's sink.
// Two sweeps: the forward one forms abar per segment, factors R_pp and forward-substitutes a_P (L, W, z to the workspace); the
// backward one back-substitutes lambda and, as soon as lambda_v and lambda_{v+1} are known, emits segment v's time gradient
// and finishes vertex v + 1's fixed-value gradient (abar and H lambda~ are formed again from u: only L, W, z are stored).
// Plain double.  The code is __host__ __device__ over plain arrays (tests/host/vjp_harness.cpp runs it on the CPU); every
// inner product is an explicit fma and contraction is off, so that the CPU and the GPU execute the same operations.
#pragma once

#include "mrs_tg_constants.h"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace vjp {

constexpr int kTri = kB * (kB + 1) / 2;
// per vertex and lane: L (diagonal entries hold 1 / L_cc), W = L^-1 E, z = L^-1 y
constexpr int kWsL = 0, kWsW = kTri, kWsZ = kWsW + kB * kB, kWsPerVertex = kWsZ + kB;

// The unit-time tables as compile-time constants: with d a template argument every table read has a constant index and is
// folded into the instruction stream (no constant-memory loads, no scalar registers held across the sweeps)
static constexpr double kAbarInv[kN][kN] = MRS_TG_ABAR_INV_INIT;
static constexpr double kHbar[kB][kN][kN] = MRS_TG_HBAR_INIT;
#define MRS_TG_VJP_ABAR kAbarInv
#define MRS_TG_VJP_HBAR kHbar

// 1 / sqrt(x), correctly rounded on both sides (a handful per vertex), where the refinement's inv_sqrt_pivot_rsq takes the
// device's approximation; a pivot <= 0 is rejected (variable left at 0)
MRS_TG_HD inline double inv_sqrt_pivot_exact(double x) {
  MRS_TG_NO_CONTRACT
  return (x > 0.0) ? 1.0 / sqrt(x) : 0.0;
}

using LaneWs = LaneWsT<kWsPerVertex>;

// The vertex derivatives the forward returned: fixed slots from fixed_values; free slots d_k = k! c_k of the segment that
// starts at the vertex, at the last vertex p^(k)(T) of the last segment (Horner)
MRS_TG_HD inline void vertex_values(const uint8_t* mask, const double* vals, const double* coeffs_path, const double* times, int v0,
                                    int S, int dim, int v, double (&x)[kB]) {
  MRS_TG_NO_CONTRACT
  constexpr double kFact[kB] = {1.0, 1.0, 2.0, 6.0, 24.0};
  const int seg = v < S ? v : S - 1;
  const double* c = coeffs_path + ((size_t)seg * kD + dim) * kN;
  // (the fixed value and the start coefficient are both loaded and one is selected: no load waits for the mask)
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) {
    const double fixed = vals[((size_t)(v0 + v) * kB + k) * kD + dim];
    const double start = c[k] * kFact[k];
    x[k] = slot_free(mask, v0 + v, k) ? start : fixed;
  }
  if (v == S) {
    const double T = times[S - 1];
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) {
      if (!slot_free(mask, v0 + v, k)) continue;
      double acc = 0.0;
      MRS_TG_UNROLL
      for (int j = kN - 1; j >= k; --j) {
        double f = 1.0;
        MRS_TG_UNROLL
        for (int m = j - k + 1; m <= j; ++m) f *= (double)m;  // j! / (j - k)!, an exact integer
        acc = fma(acc, T, c[j] * f);
      }
      x[k] = acc;
    }
  }
}

// One segment's quantities at time T: powers, H u, A^-T G and the direct term abar = A^-T G + g H u, and the parts of the time
// gradient that do not need lambda.
struct Segment {
  double tp[kB];   // T^k
  double sp[kB];   // T^(1 - 2d + k)
  double invT;
  double hu[kN];   // H u
  double abar[kN]; // A^-T G + g H u
  double t_direct; // G . dc/dT|_u + g/2 u^T H' u
};

template <int d>
MRS_TG_HD inline void seg_powers(double T, double (&tp)[kB], double (&sp)[kB]) {
  MRS_TG_NO_CONTRACT
  double td = 1.0;
  for (int k = 0; k < d; ++k) td *= T;
  const double s = T / (td * td);
  tp[0] = 1.0;
  MRS_TG_UNROLL
  for (int k = 1; k < kB; ++k) tp[k] = tp[k - 1] * T;
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) sp[k] = s * tp[k];
}

// H x = sp[s(a)] (Hbar (D_T x))_a
template <int d>
MRS_TG_HD inline void hessian_product(const double (&tp)[kB], const double (&sp)[kB], const double (&x)[kN], double (&out)[kN]) {
  MRS_TG_NO_CONTRACT
  double xh[kN];
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) xh[a] = tp[a % kB] * x[a];
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) {
    double s = 0.0;
    MRS_TG_UNROLL
    for (int b = 0; b < kN; ++b) s = fma(MRS_TG_VJP_HBAR[d][a][b], xh[b], s);
    out[a] = sp[a % kB] * s;
  }
}

template <int d>
MRS_TG_HD inline void segment_terms(double T, const double (&u)[kN], const double* G, double g, Segment& sg) {
  MRS_TG_NO_CONTRACT
  seg_powers<d>(T, sg.tp, sg.sp);
  sg.invT = 1.0 / T;
  hessian_product<d>(sg.tp, sg.sp, u, sg.hu);
  // u^T H u and sum_a s(a) u_a (H u)_a: u^T H' u = ((1 - 2d) u^T H u + 2 sum_a s(a) u_a (H u)_a) / T
  double q0 = 0.0, q1 = 0.0;
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) {
    q0 = fma(u[a], sg.hu[a], q0);
    q1 = fma((double)(a % kB) * u[a], sg.hu[a], q1);
  }
  const double t_cost = 0.5 * g * (fma((double)(1 - 2 * d), q0, 2.0 * q1) * sg.invT);
  if (G == nullptr) {
    MRS_TG_UNROLL
    for (int a = 0; a < kN; ++a) sg.abar[a] = g * sg.hu[a];
    sg.t_direct = t_cost;
    return;
  }
  // ghat_j = G_j T^-j; (A^-T G)_a = T^s(a) sum_j Abar^-1_ja ghat_j; cbar = Abar^-1 D_T u (c_j = T^-j cbar_j)
  double gh[kN], uh[kN];
  double ip = 1.0;
  MRS_TG_UNROLL
  for (int j = 0; j < kN; ++j) {
    gh[j] = G[j] * ip;
    ip *= sg.invT;
  }
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) uh[a] = sg.tp[a % kB] * u[a];
  // G . dc/dT|_u = (sum_a s(a) u_a (A^-T G)_a - sum_j j G_j c_j) / T
  double p0 = 0.0, p1 = 0.0;
  MRS_TG_UNROLL
  for (int j = 0; j < kN; ++j) {
    double cb = 0.0;
    MRS_TG_UNROLL
    for (int a = 0; a < kN; ++a) cb = fma(MRS_TG_VJP_ABAR[j][a], uh[a], cb);
    p1 = fma((double)j * gh[j], cb, p1);
  }
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) {
    double bh = 0.0;
    MRS_TG_UNROLL
    for (int j = 0; j < kN; ++j) bh = fma(MRS_TG_VJP_ABAR[j][a], gh[j], bh);
    const double atg = sg.tp[a % kB] * bh;
    sg.abar[a] = fma(g, sg.hu[a], atg);
    p0 = fma((double)(a % kB) * u[a], atg, p0);
  }
  sg.t_direct = (p0 - p1) * sg.invT + t_cost;
}

// lambda~^T H' u = ((1 - 2d) lambda~^T H u + sum_a s(a) lambda~_a (H u)_a + sum_b s(b) u_b (H lambda~)_b) / T
template <int d>
MRS_TG_HD inline double lambda_term(const Segment& sg, const double (&u)[kN], const double (&lam)[kN], const double (&hl)[kN]) {
  MRS_TG_NO_CONTRACT
  double r0 = 0.0, r1 = 0.0;
  MRS_TG_UNROLL
  for (int a = 0; a < kN; ++a) {
    r0 = fma(lam[a], sg.hu[a], r0);
    r1 = fma((double)(a % kB) * lam[a], sg.hu[a], r1);
    r1 = fma((double)(a % kB) * u[a], hl[a], r1);
  }
  return fma((double)(1 - 2 * d), r0, r1) * sg.invT;
}

// The whole backward pass of one lane.  coeffs_path / grad_coeffs_path: segment i, this dimension at [(i * kD + dim) * kN + k]
// (grad_coeffs_path NULL: G = 0); g: dL/dJ of the path; grad_vals: the caller's [sum V][5][4] array (NULL: not written), this
// lane's column of vertices v0 .. v0 + S; time_sink(i, x): this dimension's share of dL/dT_i, segments S-1 .. 0 in turn.
template <int d, class TimeSink>
MRS_TG_HD inline void vjp_lane_d(const uint8_t* mask, const double* vals, int v0, int S, int dim, const double* times,
                               const double* coeffs_path, const double* grad_coeffs_path, double g, const LaneWs& w,
                               double* grad_vals, TimeSink&& time_sink) {
  MRS_TG_NO_CONTRACT
  // ---- forward sweep: abar per segment, factor R_pp, z = L^-1 (a_P - W_{v-1}^T z_{v-1}) --------------------------------
  {
    double Sm[kTri], carry[kB], zprev[kB], Wp[kB * kB], ds[kB], de[kB];
    MRS_TG_UNROLL
    for (int e = 0; e < kTri; ++e) Sm[e] = 0.0;
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) carry[k] = zprev[k] = 0.0;
    MRS_TG_UNROLL
    for (int e = 0; e < kB * kB; ++e) Wp[e] = 0.0;
    vertex_values(mask, vals, coeffs_path, times, v0, S, dim, 0, ds);
    for (int v = 0; v <= S; ++v) {
      const unsigned fs = free_bits(mask, v0 + v);
      const unsigned fe = v < S ? free_bits(mask, v0 + v + 1) : 0u;
      double a[kB];
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) a[k] = carry[k];
      double p2[9];  // H(r, c) = Hbar[r][c] T^(1 - 2d + r % 5 + c % 5)
      if (v < S) {
        vertex_values(mask, vals, coeffs_path, times, v0, S, dim, v + 1, de);
        double u[kN];
        MRS_TG_UNROLL
        for (int k = 0; k < kB; ++k) {
          u[k] = ds[k];
          u[kB + k] = de[k];
        }
        Segment sg;
        segment_terms<d>(times[v], u, grad_coeffs_path ? grad_coeffs_path + ((size_t)v * kD + dim) * kN : nullptr, g, sg);
        MRS_TG_UNROLL
        for (int k = 0; k < kB; ++k) {
          a[k] = carry[k] + sg.abar[k];
          carry[k] = sg.abar[kB + k];
        }
        p2[0] = sg.sp[0];
        MRS_TG_UNROLL
        for (int m = 1; m < 9; ++m) p2[m] = p2[m - 1] * times[v];
        MRS_TG_UNROLL
        for (int r = 0; r < kB; ++r)
          MRS_TG_UNROLL
          for (int c = 0; c <= r; ++c) Sm[tri5(r, c)] = fma(MRS_TG_VJP_HBAR[d][r][c], p2[r + c], Sm[tri5(r, c)]);
      }
      // mask, factor (gen_factor's rule: constrained slots get a unit row and a zero right-hand side)
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
        const double inv = inv_sqrt_pivot_exact(dsum);
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
      // forward substitution on vertex v (Wp, zprev: vertex v - 1's, zero at v = 0)
      double z[kB];
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) {
        double s = a[k];
        MRS_TG_UNROLL
        for (int m = 0; m < kB; ++m) s = fma(-Wp[m * kB + k], zprev[m], s);
        s = ((fs >> k) & 1u) ? s : 0.0;
        MRS_TG_UNROLL
        for (int m = 0; m < k; ++m) s = fma(-L[tri5(k, m)], z[m], s);
        z[k] = s * Linv[k];
      }
      MRS_TG_UNROLL
      for (int r = 0; r < kB; ++r)
        MRS_TG_UNROLL
        for (int c = 0; c <= r; ++c) w.at(v, kWsL + tri5(r, c)) = (r == c) ? Linv[r] : L[tri5(r, c)];
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) {
        w.at(v, kWsZ + k) = z[k];
        zprev[k] = z[k];
      }
      if (v == S) {  // the last vertex couples to nothing: its W block is zero, written so that no sweep reads undefined memory
        MRS_TG_UNROLL
        for (int e = 0; e < kB * kB; ++e) w.at(v, kWsW + e) = 0.0;
        break;
      }
      // W = L^-1 E, E = coupling block restricted to (free here) x (free at the next vertex)
      MRS_TG_UNROLL
      for (int c = 0; c < kB; ++c)
        MRS_TG_UNROLL
        for (int r = 0; r < kB; ++r) {
          const bool on = ((fs >> r) & 1u) && ((fe >> c) & 1u);
          double s = on ? MRS_TG_VJP_HBAR[d][r][kB + c] * p2[r + c] : 0.0;
          MRS_TG_UNROLL
          for (int m = 0; m < r; ++m) s = fma(-L[tri5(r, m)], Wp[m * kB + c], s);
          Wp[r * kB + c] = s * Linv[r];
        }
      MRS_TG_UNROLL
      for (int e = 0; e < kB * kB; ++e) w.at(v, kWsW + e) = Wp[e];
      // Schur complement on the next vertex
      MRS_TG_UNROLL
      for (int r = 0; r < kB; ++r)
        MRS_TG_UNROLL
        for (int c = 0; c <= r; ++c) {
          double s = MRS_TG_VJP_HBAR[d][kB + r][kB + c] * p2[r + c];
          MRS_TG_UNROLL
          for (int m = 0; m < kB; ++m) s = fma(-Wp[m * kB + r], Wp[m * kB + c], s);
          Sm[tri5(r, c)] = s;
        }
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) ds[k] = de[k];
    }
  }
  // ---- backward sweep: lambda_v = L^-T (z_v - W_v lambda_{v+1}); segment v's time gradient; vertex v + 1's d_F gradient --
  double xn[kB], carry_a[kB], carry_r[kB], de[kB];
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) xn[k] = carry_a[k] = carry_r[k] = 0.0;
  vertex_values(mask, vals, coeffs_path, times, v0, S, dim, S, de);
  for (int v = S; v >= 0; --v) {
    double L[kTri], W[kB * kB], z[kB];
    MRS_TG_UNROLL
    for (int e = 0; e < kTri; ++e) L[e] = w.at(v, kWsL + e);
    MRS_TG_UNROLL
    for (int e = 0; e < kB * kB; ++e) W[e] = w.at(v, kWsW + e);
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) z[k] = w.at(v, kWsZ + k);
    const unsigned fb = free_bits(mask, v0 + v);
    double t[kB], x[kB];
    MRS_TG_UNROLL
    for (int r = 0; r < kB; ++r) {
      double s = z[r];
      MRS_TG_UNROLL
      for (int c = 0; c < kB; ++c) s = fma(-W[r * kB + c], xn[c], s);  // (v = S: xn = 0)
      t[r] = s;
    }
    MRS_TG_UNROLL
    for (int r = kB - 1; r >= 0; --r) {
      double s = t[r];
      MRS_TG_UNROLL
      for (int m = r + 1; m < kB; ++m) s = fma(-L[tri5(m, r)], x[m], s);
      x[r] = ((fb >> r) & 1u) ? s * L[tri5(r, r)] : 0.0;
    }
    if (v < S) {
      double ds[kB];
      vertex_values(mask, vals, coeffs_path, times, v0, S, dim, v, ds);
      double u[kN], lam[kN];
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) {
        u[k] = ds[k];
        u[kB + k] = de[k];
        lam[k] = x[k];
        lam[kB + k] = xn[k];
      }
      Segment sg;
      segment_terms<d>(times[v], u, grad_coeffs_path ? grad_coeffs_path + ((size_t)v * kD + dim) * kN : nullptr, g, sg);
      double hl[kN];
      hessian_product<d>(sg.tp, sg.sp, lam, hl);
      time_sink(v, sg.t_direct - lambda_term<d>(sg, u, lam, hl));
      const unsigned fn = free_bits(mask, v0 + v + 1);
      MRS_TG_UNROLL
      for (int k = 0; k < kB; ++k) {
        const double ak = sg.abar[kB + k] + carry_a[k];
        const double rk = hl[kB + k] + carry_r[k];
        if (grad_vals) grad_vals[((size_t)(v0 + v + 1) * kB + k) * kD + dim] = ((fn >> k) & 1u) ? 0.0 : ak - rk;
        carry_a[k] = sg.abar[k];
        carry_r[k] = hl[k];
        de[k] = ds[k];
      }
    }
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) xn[k] = x[k];
  }
  const unsigned f0 = free_bits(mask, v0);
  if (grad_vals) {
    MRS_TG_UNROLL
    for (int k = 0; k < kB; ++k) grad_vals[((size_t)v0 * kB + k) * kD + dim] = ((f0 >> k) & 1u) ? 0.0 : carry_a[k] - carry_r[k];
  }
}

// d = 0 .. 4 (the caller checks the range), each instantiated with its own constants
template <class TimeSink>
MRS_TG_HD inline void vjp_lane(const uint8_t* mask, const double* vals, int v0, int S, int d, int dim, const double* times,
                               const double* coeffs_path, const double* grad_coeffs_path, double g, const LaneWs& w,
                               double* grad_vals, TimeSink&& time_sink) {
  switch (d) {
    case 0: vjp_lane_d<0>(mask, vals, v0, S, dim, times, coeffs_path, grad_coeffs_path, g, w, grad_vals, time_sink); break;
    case 1: vjp_lane_d<1>(mask, vals, v0, S, dim, times, coeffs_path, grad_coeffs_path, g, w, grad_vals, time_sink); break;
    case 2: vjp_lane_d<2>(mask, vals, v0, S, dim, times, coeffs_path, grad_coeffs_path, g, w, grad_vals, time_sink); break;
    case 3: vjp_lane_d<3>(mask, vals, v0, S, dim, times, coeffs_path, grad_coeffs_path, g, w, grad_vals, time_sink); break;
    default: vjp_lane_d<4>(mask, vals, v0, S, dim, times, coeffs_path, grad_coeffs_path, g, w, grad_vals, time_sink); break;
  }
}

}  // namespace vjp
}  // namespace mrs_tg

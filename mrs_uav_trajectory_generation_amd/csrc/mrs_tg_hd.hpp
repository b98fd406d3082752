// mrs_tg_hd.hpp -- what the host-checkable kernel headers share (mrs_tg_refine.hpp, mrs_tg_vjp.hpp, mrs_tg_maxima_vjp.hpp,
// mrs_tg_sample_vjp.hpp, mrs_tg_evaluate.hpp, mrs_tg_deviation.hpp, mrs_tg_estimate_vjp.hpp, mrs_tg_passage.hpp, mrs_tg_baca.hpp, mrs_tg_fallback.hpp, mrs_tg_pathedit.hpp, mrs_tg_heading.hpp, mrs_tg_initial.hpp, mrs_tg_request.hpp) and the device headers take their shape constants from.
// Plain C++17 without a HIP include: hipcc compiles it for both sides, g++ compiles it for the harnesses under tests/host/,
// which run the same headers on the CPU.  DESIGN.md section 4a states the convention these headers follow.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MRS_TG_HD __host__ __device__
#else
#define MRS_TG_HD
#endif
// MRS_TG_NO_CONTRACT at the top of a function body: no product of that body is contracted into a fused multiply-add, the
// fused steps are the explicit fma calls (g++ gets -ffp-contract=off from the harness build)
#if defined(__clang__)
#define MRS_TG_NO_CONTRACT _Pragma("clang fp contract(off)")
#define MRS_TG_UNROLL _Pragma("unroll")
#else
#define MRS_TG_NO_CONTRACT
#define MRS_TG_UNROLL
#endif

namespace mrs_tg {

constexpr int kN = 10;         // coefficients per polynomial
constexpr int kD = 4;          // dimensions
constexpr int kB = 5;          // derivative slots per vertex: the side of a vertex block
constexpr int kMaxOrders = 5;  // derivative orders 0..4 of a full state row

// j!/(j-k)!, an exact integer; a compile-time constant wherever j and k are
MRS_TG_HD constexpr double falling_factorial(int j, int k) {
  double v = 1.0;
  for (int n = 0; n < k; ++n) v *= (double)(j - n);
  return v;
}
static_assert(falling_factorial(9, 4) == 3024.0 && falling_factorial(9, 0) == 1.0 && falling_factorial(4, 4) == 24.0 &&
                  falling_factorial(3, 4) == 0.0,
              "j!/(j-k)!, 0 for k > j");

// The same value from a loop of constant trip count with a predicate: the form the sampler's backward pass is written in
// (mrs_tg_sample_vjp.hpp), where j or k is a lane's run-time value and the weights are to stay in registers.  With the loop
// above in its place the compiler builds another sample_vjp_kernel, so the two stay two.
MRS_TG_HD inline double falling_factorial_predicated(int j, int k) {
  double v = 1.0;
  MRS_TG_UNROLL
  for (int n = 0; n < kN; ++n)
    if (n < k) v *= (double)(j - n);
  return v;
}

// the heading of order 0 brought into [-pi, pi]: the nearest multiple of 2 pi taken off in two pieces
MRS_TG_HD inline double wrap_heading(double y) {
  const double two_pi_hi = 6.283185307179586232e+00, two_pi_lo = 2.449293598294706414e-16;
  const double kf = rint(y * 1.591549430918953456e-01);
  return fma(-kf, two_pi_lo, fma(-kf, two_pi_hi, y));
}

// every accumulator of the backward passes: acc <- acc + term, from 0.0
MRS_TG_HD inline double accumulate(double acc, double term) {
  MRS_TG_NO_CONTRACT
  return acc + term;
}

// index into a packed lower-triangular 5 x 5 (r >= c)
MRS_TG_HD constexpr int tri5(int r, int c) { return r * (r + 1) / 2 + c; }
static_assert(tri5(0, 0) == 0 && tri5(4, 4) == kB * (kB + 1) / 2 - 1, "packed lower triangle");

// the constraint mask [vertex][5]: 0 = the slot is free
MRS_TG_HD inline bool slot_free(const uint8_t* mask, int v, int k) { return mask[(size_t)v * kB + k] == 0; }
MRS_TG_HD inline unsigned free_bits(const uint8_t* mask, int v) {
  unsigned f = 0u;
  MRS_TG_UNROLL
  for (int k = 0; k < kB; ++k) f |= slot_free(mask, v, k) ? (1u << k) : 0u;
  return f;
}

// Where a lane's per-vertex state lives: element e of vertex v at ws[(v * PerVertex + e) * stride] (the kernel strides by the
// number of lanes so that a wavefront's accesses coalesce; the host harness passes stride 1).  PerVertex is the family's own
// record size: the refinement keeps two double-double iterates per vertex beside the factors, the solve's backward pass does not.
template <int PerVertex>
struct LaneWsT {
  double* ws;
  size_t stride;
  MRS_TG_HD double& at(int v, int e) const { return ws[((size_t)v * PerVertex + e) * stride]; }
};

}  // namespace mrs_tg

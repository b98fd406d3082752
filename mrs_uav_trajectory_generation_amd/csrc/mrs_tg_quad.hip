// mrs_tg_quad.hip -- the linear QP solve for SATURATED devices: four lanes per path, the factors of the block elimination in LDS.
//
// What it replaces: PolynomialOptimization::updateSegmentTimes + constructR + solveLinear +
// updateSegmentsFromCompactConstraints + computeCost for every path of a batch
// (/root/reference/include/eth_trajectory_generation/impl/polynomial_optimization_linear_impl.h:289-304, 311-373,
// 264-282, 128-141) -- the same contract as mrs_tg_rows.hip, chosen by the launcher once a launch carries more paths than
// the device has wavefront slots for the rows kernel.
//
// Why a second solve kernel.  solve_rows_kernel spends a whole wavefront on one or two paths (one lane per unknown, rank-one
// updates by DPP row broadcasts): the shortest dependent chain there is, ~1900 wavefront instructions per path -- 3 % of the
// lanes carry useful work.  With 65536 paths every SIMD sees 64 of them one after the other, and the solve is bound by that
// instruction count (202 us).  Here a quad of lanes owns a path (lane = dimension) and runs the block-tridiagonal Cholesky of
// the vertex chain sequentially: 16 paths per wavefront, ~5000 wavefront instructions for all of them -- ~300 per path.  What
// made the four-lanes-per-path kernel of round 1 slow was its factor store (L, W, z of every vertex, written for the back
// substitution) in global memory: 30 doubles per vertex and LANE, 250 MB out and back in at 65536 x 10.  Here the store is in
// LDS, once per PATH (the four lanes of a quad hold the same L: lane 0 writes it, every lane its own z; W is formed again in
// the back substitution instead of being kept): 26 doubles per vertex, 31 KB per wavefront at 10 segments, five wavefronts
// per CU.  Barely more than one wavefront per SIMD -- a step's latencies are exposed, so positions are requested three
// segments ahead -- and still a multiple of the rows kernel's throughput.
//
//   prologue  segment times -> LDS (the feasibility scaling of a Mellinger pipeline's last solve applied on the way);
//             is every path of the wavefront "plain" (start | interior ... | end: position-only interior vertices, fully
//             constrained ends at rest)?
//   plain     forward: per segment near block + factor + W + Schur complement, all from the exact unit-time constants times
//             powers of T (as FastStep::interior_t); backward: x_v = L^-T (z - W x_{v+1}), c = A^-1 d segment by segment,
//             cost 0.5 c^T Q c as the reference computes it
//   other     the general masked step of mrs_tg_solve.hpp::solve_path (factors in the plan's global workspace)
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "mrs_tg_device.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_nl_common.hpp"
#include "mrs_tg_solve.hpp"

// wavefronts per SIMD the kernels are compiled for.  The single launch keeps its 262 registers (one wavefront per SIMD; LDS
// would allow 1.25): at 65536 x 10 the two-wavefront build is 8 % slower (137 vs 127 us, 20 B of scratch).  The grouped launch
// is compiled for two (256 VGPRs + 12 B): a host that keeps several dispatches in flight then has 1280 instead of 1024
// wavefront slots for them -- grouped headline over 200 steps 485 -> 539-556 M/s, over 20 steps 339 -> 345-357 with ten
// steps per dispatch and twenty batches in flight.
#ifndef MRS_TG_QUAD_WAVES
#define MRS_TG_QUAD_WAVES 1
#endif
#ifndef MRS_TG_QUAD_GROUP_WAVES
#define MRS_TG_QUAD_GROUP_WAVES 2
#endif
// The two-sided group kernel: two as well.  Its 18.5 KB of LDS per wavefront (10 segments) let a CU hold eight wavefronts -- two
// per SIMD -- whatever the register budget says, so a build for three (168 registers: the plain path fits, the general step
// spills) only pays for the registers: 25.9 us per dispatch against 24.4, the region 67-69 us against 63 (same box, alternating
// runs; profiles/round6_duo_group_waves_ab.txt).  One wavefront of this kernel keeps its SIMD's FP64 pipe about half busy (an
// FMA on three vector registers issues every 8.7 clocks from one wavefront: profiles/round6_issue_latencies.txt).
#ifndef MRS_TG_DUO_GROUP_WAVES
#define MRS_TG_DUO_GROUP_WAVES 2
#endif

namespace mrs_tg {

// (kQdPaths, 16 paths per wavefront; the record's size kQdRec; quad_lds_doubles: mrs_tg_solve_route.hpp)
// LDS record of (vertex, path): L off-diagonal [6] | 1 / diag L [4] | z [4 rows][4 dimensions].  W = L^-1 E is NOT kept: the
// back substitution forms W x_{v+1} as L^-1 (E x_{v+1}) from the segment's time again (~25 instructions more per vertex,
// 16 doubles less per record: five wavefronts per CU instead of three at 10 segments)
constexpr int kQdL = 0, kQdLinv = 6, kQdZ = 10;
static_assert(kQdZ + 4 * kD == kQdRec, "the record fills its size");

// T^(m + 1 - 2d), m = 0..8, the objective order as select masks (no branch tree per segment)
__device__ __forceinline__ void quad_powers(double T, bool d1, bool d2, bool d4, double (&p2)[9]) {
  const double t2 = T * T;
  const double t4 = t2 * t2;
  const double td = ((d1 ? T : 1.0) * (d2 ? t2 : 1.0)) * (d4 ? t4 : 1.0);
  p2[0] = T * rcp_refined(td * td);
  p2[1] = p2[0] * T;
  p2[2] = p2[0] * t2;
  p2[3] = p2[1] * t2;
  p2[4] = p2[0] * t4;
  p2[5] = p2[1] * t4;
  p2[6] = p2[2] * t4;
  p2[7] = p2[3] * t4;
  p2[8] = p2[4] * t4;
}

// a pair of coefficients (16 bytes), an ordinary store.  As a streaming store (an experiment build) -- measured in round 6 after
// the samples and the assembled blocks had gained from it: here it is 2.5-3 x SLOWER (headline dispatch 26 -> 73-81 us, 65536 x 10
// 131 -> 335-339 us).  That trial is about SEPARATE 16-BYTE PIECES: a lane owned 80 consecutive bytes then, so a store instruction
// wrote 64 of them, and without the L2 to combine them every piece is a partial-line write to HBM.  It says nothing about a store
// instruction that writes 64 consecutive bytes per segment (store_coeff_pair_through below); it does say that a store of separate
// pieces must stay an ordinary one.
__device__ __forceinline__ void store_coeff_pair(double2* dst, double a, double b) {
  *dst = make_double2(a, b);
}

// The same 16 bytes as a store that leaves the XCD's L2 at once instead of staying there as a dirty line until the release at the
// end of the dispatch writes all of them back.  Only where the lanes of a store instruction write
// 64 consecutive bytes per segment (the exchange road of solve_duo_body), and only in a dispatch whose coefficients no kernel
// reads next: the line does not stay in L2.  MRS_TG_DUO_THROUGH_FORM (experiment builds: the A/B of profiles/duo_store_through_ab.txt):
// 1 = write-through at agent scope (sc1; the default), 2 = at system scope (sc0 sc1), 3 = the compiler's non-temporal store (nt).
// (inline assembly: the compiler has no 16-byte store with these cache bits to lower to.  It reads registers only -- no memory
// clobber, the LDS reads around it keep their schedule; the closing s_nop keeps the compiler's next instruction off the data
// registers until the store has read them.  The compiler does not count it in vmcnt: its own waits are then stricter than
// needed, never weaker, and there is no load behind these stores.)
#ifndef MRS_TG_DUO_THROUGH_FORM
#define MRS_TG_DUO_THROUGH_FORM 1
#endif
// (BYTES: the instruction's offset field, so that the five stores of a step share one address register pair)
template <int BYTES>
__device__ __forceinline__ void store_coeff_pair_through(double2* dst, double2 v) {
  typedef int int4v __attribute__((ext_vector_type(4)));
  const int4v bits = __builtin_bit_cast(int4v, v);
#if MRS_TG_DUO_THROUGH_FORM == 3
  __builtin_nontemporal_store(bits, reinterpret_cast<int4v*>(dst + BYTES / 16));
#else
#if MRS_TG_DUO_THROUGH_FORM == 2
  asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc0 sc1\n\ts_nop 1" ::"v"(dst), "v"(bits), "i"(BYTES));
#else
  asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" ::"v"(dst), "v"(bits), "i"(BYTES));
#endif
#endif
}

// The same store with its address as a wave-uniform base and a 32-bit byte offset per lane (the lean instantiation of the grouped
// kernel: the base is the wavefront's first segment, so no 64-bit address is formed per lane and step).  Same bytes, same place.
template <int BYTES>
__device__ __forceinline__ void store_coeff_pair_through(const double* base, unsigned lane_bytes, double2 v) {
  typedef int int4v __attribute__((ext_vector_type(4)));
  const int4v bits = __builtin_bit_cast(int4v, v);
#if MRS_TG_DUO_THROUGH_FORM == 3
  __builtin_nontemporal_store(bits, reinterpret_cast<int4v*>(reinterpret_cast<char*>(const_cast<double*>(base)) + lane_bytes + BYTES));
#else
#if MRS_TG_DUO_THROUGH_FORM == 2
  asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc0 sc1\n\ts_nop 1" ::"v"(lane_bytes), "v"(bits), "s"(base), "i"(BYTES));
#else
  asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc1\n\ts_nop 1" ::"v"(lane_bytes), "v"(bits), "s"(base), "i"(BYTES));
#endif
#endif
}

__device__ __forceinline__ double quad_sum(double v) {  // over the four lanes of a quad, to all of them
  v += dpp_move<0xB1>(v);
  v += dpp_move<0x4E>(v);
  return v;
}

// WP: vertex positions from the compact waypoint array (MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS).  A template parameter, not a
// run-time stride: with the stride in a register the value-array path lost 13 % (65536 x 10: 129 -> 147 us, same box)
// ENDS: the two end vertices may leave derivative slots free (rest-to-rest paths under an objective order below snap: jerk and
// / or snap are unknowns there).  Such an end vertex is eliminated like an interior one -- its block is the near (far) part of
// its only segment with the identity in the rows and columns of the constrained slots and zero in place of their reciprocal
// pivots, so that they contribute nothing to W, z and x -- and has a record of its own: records for vertices 0 .. S instead
// of 1 .. S - 1.  A fully constrained end takes the plain path's step.  Without ENDS such paths take the general step.
// MOVING: a START vertex whose constrained derivatives carry non-zero values (a path that starts from a moving state) stays on
// the fast road -- the single-launch kernels; the grouped launch (the headline's kernel) is compiled without it: the lines
// below cost it 16 % (330 -> 300 M/s over 20 steps, 556 -> 469 over 200, same box) although no wavefront of it ever takes them
template <bool WP, bool ENDS = false, bool MOVING = false>
__device__ __forceinline__ void solve_quad_body(const BatchView& b, int d, const uint8_t* __restrict__ mask,
                                                const double* __restrict__ vals, const double* seg_times,
                                                double* __restrict__ coeffs, int32_t* __restrict__ status,
                                                double* __restrict__ cost, const int32_t* __restrict__ status_in, double* ws,
                                                const RowsTail& tail, int block, const double* __restrict__ pos_wp) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, pl = lane >> 2, dim = lane & 3;
  const int q = block * kQdPaths + pl;
  const bool active = q < b.n_paths;
  const PathRef pr = path_at(b, active ? q : b.n_paths - 1);
  const int S = pr.S;
  const int Smax = b.max_segments;
  double* rec0 = lds;
  double* tbuf = lds + (size_t)(ENDS ? Smax + 1 : (Smax > 1 ? Smax - 1 : 1)) * kQdRec * kQdPaths;  // [segment][path]
  unsigned char* vmask = reinterpret_cast<unsigned char*>(tbuf + (size_t)Smax * kQdPaths);        // ENDS: [vertex][path] free masks
  // ---- prologue: times (scaled, for the last solve of a Mellinger pipeline), plainness of the path
  const bool scaling = tail.maxima != nullptr;
  double t_sum = 0.0;
  bool ok = S >= 2, pos_ok = true;
  unsigned fm_first = 0u, fm_last = 0u;  // ENDS: free slots of the two end vertices (bit r: derivative r + 1)
  bool moving_path = false;              // the start vertex's constrained derivatives carry non-zero values (lane 0 of the quad knows)
  if (active) {
    const int opt_st = scaling ? tail.opt_status[pr.p] : 0;
    for (int i = dim; i < S; i += 4) {
      double T = seg_times[pr.s0 + i];
      if (scaling) {  // scaleSegmentTimesToMeetConstraints (trajectory.cpp:625-657), then the solve at the scaled times
        if (opt_st != -2) T *= violation_scaling(tail.maxima + (size_t)(pr.s0 + i) * 9, tail.limits + (size_t)pr.p * 9);
        tail.seg_times_out[pr.s0 + i] = T;
      }
      tbuf[i * kQdPaths + pl] = T;
      t_sum += T;
    }
    for (int v = dim; v <= S; v += 4) {
      const uint8_t* mrow = mask + (size_t)(pr.v0 + v) * kHalf;
      const bool end = v == 0 || v == S;
      unsigned fixed = 0;
#pragma unroll
      for (int k = 0; k < kHalf; ++k) fixed |= (mrow[k] != 0 ? 1u : 0u) << k;
      pos_ok = pos_ok && (fixed & 1u);
      if (end) {
        const double* vrow = vals + (size_t)(pr.v0 + v) * kHalf * kD;
        double nz = 0.0;
        // (the values of unconstrained slots are not read by anybody: only those of constrained ones count.  Every value is
        // LOADED unconditionally, sixteen requests back to back -- written as a conditional expression around the load they
        // became four branches with a trip to memory each: 65536 x 10 132 -> 147 us, the grouped headline -16 %)
        double av[kHalf * kD];
#pragma unroll
        for (int e = kD; e < kHalf * kD; ++e) av[e] = fabs(vrow[e]);
#pragma unroll
        for (int k = 1; k < kHalf; ++k)
#pragma unroll
          for (int e = 0; e < kD; ++e) nz += ((fixed >> k) & 1u) ? av[k * kD + e] : 0.0;
        // a START vertex whose constrained derivatives carry non-zero values (a path that starts from a moving state) stays on
        // this road: the values are right-hand-side terms of the first step (below); the end vertex must be at rest
        if (MOVING && v == 0) {
          moving_path = nz != 0.0;
          nz = 0.0;
        }
        if (ENDS) {
          ok = ok && (fixed & 1u) && nz == 0.0;
          if (v == 0) fm_first = (~fixed >> 1) & 0xFu;
          if (v == S) fm_last = (~fixed >> 1) & 0xFu;
        } else {
          ok = ok && fixed == 0x1Fu && nz == 0.0;
        }
      } else if (ENDS) {
        // an interior vertex may hold slots constrained to ZERO (a stop_at vertex: velocity = acceleration = jerk = 0): it is
        // eliminated with the identity in those slots; its values are looked at only when it has such slots
        bool zero = true;
        if (fixed != 0x1u) {
          const double* vrow = vals + (size_t)(pr.v0 + v) * kHalf * kD;
          double av[kHalf * kD];
#pragma unroll
          for (int e = kD; e < kHalf * kD; ++e) av[e] = fabs(vrow[e]);
          double nz = 0.0;
#pragma unroll
          for (int k = 1; k < kHalf; ++k)
#pragma unroll
            for (int e = 0; e < kD; ++e) nz += ((fixed >> k) & 1u) ? av[k * kD + e] : 0.0;
          zero = nz == 0.0;
        }
        ok = ok && (fixed & 1u) && zero;
      } else {
        ok = ok && fixed == 0x1u;
      }
      if (ENDS) vmask[v * kQdPaths + pl] = (unsigned char)((~fixed >> 1) & 0xFu);
    }
  }
  if (ENDS) {  // vertex 0 was read by lane 0 of the quad, vertex S by lane S mod 4
    fm_first = (unsigned)__shfl((int)fm_first, lane & ~3, 64);
    fm_last = (unsigned)__shfl((int)fm_last, (lane & ~3) + (S & 3), 64);
  }
  t_sum = quad_sum(t_sum);
  const bool any_moving = MOVING && __ballot(active && moving_path) != 0ull;  // (wave-uniform: a wavefront of paths at rest skips every line of it)
  if (any_moving) moving_path = __shfl((int)moving_path, lane & ~3, 64) != 0;
  const bool plain_wave = __ballot(active && !ok) == 0ull;
  const unsigned long long pos_bad = __ballot(active && !pos_ok);
  const bool path_pos_ok = ((pos_bad >> (lane & ~3)) & 0xFull) == 0ull;
  wave_lds_barrier();

  double my_cost = 0.0;
  if (plain_wave) {
    // ---- the exact unit-time constants of this objective order (uniform: scalar loads)
    const double (*hb)[kN] = c_hbar[d];
    double cNear[10], cCpl[kNB][kNB], cFar[10], cN[kNB], cF[kNB];
#pragma unroll
    for (int r = 0; r < kNB; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        cNear[tri(r, c)] = hb[kSlot0 + r][kSlot0 + c];
        cFar[tri(r, c)] = hb[kHalf + kSlot0 + r][kHalf + kSlot0 + c];
      }
#pragma unroll
      for (int c = 0; c < kNB; ++c) cCpl[r][c] = hb[kSlot0 + r][kHalf + kSlot0 + c];
      cN[r] = hb[kSlot0 + r][0];
      cF[r] = hb[kHalf + kSlot0 + r][0];
    }
    const bool d1 = (d & 1) != 0, d2 = (d & 2) != 0, d4 = (d & 4) != 0;
    const int Sw = __builtin_amdgcn_readfirstlane(S);  // (a wavefront's paths may differ in length: ragged batches)
    int Smx = Sw;
    {  // longest path of the wavefront
      int s = active ? S : 0;
      for (int off = 32; off >= 4; off >>= 1) s = max(s, __shfl_xor(s, off, 64));
      Smx = __builtin_amdgcn_readfirstlane(s);
    }
    // position of vertex v, this dimension: pv[v * pstride].  From the caller's value array that is 8 bytes out of every 160
    // (and whole cache lines come along: 137 MB read for 45 MB of inputs at 65536 x 10); under
    // MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS from the compact [vertex][4] waypoint array, whose every byte is used
    const double* pv = WP ? pos_wp + (size_t)pr.v0 * kD + dim : vals + (size_t)pr.v0 * kHalf * kD + dim;
    constexpr size_t pstride = WP ? (size_t)kD : (size_t)(kHalf * kD);
    // ---- forward: block Cholesky over the vertex chain
    double Sm[10], y[kNB];
    // positions are requested three segments ahead: with less than one wavefront per SIMD nothing else hides a trip to memory,
    // and a segment step is shorter than one
    auto pos = [&](int v) { return (active && v <= S) ? pv[(size_t)v * pstride] : 0.0; };
    double p_cur = pos(0), p_nxt = pos(1), p_a2 = pos(2), p_a3 = pos(3);
    for (int i = 0; i < Smx; ++i) {
      const bool on = active && i < S;
      const double T = on ? tbuf[i * kQdPaths + pl] : 1.0;
      const double p_a4 = pos(i + 4);
      double p2[9];
      quad_powers(T, d1, d2, d4, p2);
      const double dp = p_cur - p_nxt;
      // a moving start: this dimension's constrained derivative values of the start vertex (zero in free slots), from the
      // caller's value array -- read here and again for the first segment's coefficients, not kept in between
      double f0[kNB] = {0.0, 0.0, 0.0, 0.0};
      if (any_moving && i == 0 && active && moving_path) {
        const double* vrow0 = vals + (size_t)pr.v0 * kHalf * kD + dim;
#pragma unroll
        for (int r = 0; r < kNB; ++r) f0[r] = vrow0[(r + 1) * kD];
#pragma unroll
        for (int r = 0; r < kNB; ++r) f0[r] = (!ENDS || !((fm_first >> r) & 1u)) ? f0[r] : 0.0;
      }
      if (on) {
        // ENDS: the free mask of the vertex this step eliminates: the start vertex's (0: fully constrained, nothing to
        // eliminate) or vertex i's (0xF unless it is a stop_at vertex)
        const unsigned fmv = !ENDS ? 0xFu : (i == 0 ? fm_first : (unsigned)vmask[i * kQdPaths + pl]);
        const bool free_start = ENDS && i == 0 && fm_first != 0u;
        const bool masked_step = ENDS && (i == 0 ? fm_first != 0u : fmv != 0xFu);
        if (i == 0 && !free_start) {  // the start vertex is fully constrained: the state moves to vertex 1
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
#pragma unroll
            for (int c = 0; c <= r; ++c) Sm[tri(r, c)] = cFar[tri(r, c)] * p2[r + c + 2];
            y[r] = -((cF[r] * p2[r + 1]) * dp);
          }
        } else {
          // vertex i: its block and right-hand side are complete with this segment's near part
          // (a start vertex with free slots: the near part IS its block -- the identity in the constrained slots)
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
#pragma unroll
            for (int c = 0; c <= r; ++c)
              Sm[tri(r, c)] = free_start ? cNear[tri(r, c)] * p2[r + c + 2] : fma(cNear[tri(r, c)], p2[r + c + 2], Sm[tri(r, c)]);
            y[r] = free_start ? -((cN[r] * p2[r + 1]) * dp) : fma(-(cN[r] * p2[r + 1]), dp, y[r]);
          }
          if (ENDS && free_start && any_moving) {  // the start vertex's own unknowns see its constrained values
#pragma unroll
            for (int r = 0; r < kNB; ++r)
#pragma unroll
              for (int c = 0; c < kNB; ++c)
                y[r] = fma(-(cNear[r >= c ? tri(r, c) : tri(c, r)] * p2[r + c + 2]), f0[c], y[r]);
          }
          double rs[kNB];  // ENDS: 0 in place of the reciprocal pivot of a constrained slot
#pragma unroll
          for (int r = 0; r < kNB; ++r) rs[r] = (masked_step && !((fmv >> r) & 1u)) ? 0.0 : 1.0;
          if (masked_step) {
#pragma unroll
            for (int r = 0; r < kNB; ++r)
#pragma unroll
              for (int c = 0; c <= r; ++c)
                if (!((fmv >> r) & 1u) || !((fmv >> c) & 1u)) Sm[tri(r, c)] = (r == c) ? 1.0 : 0.0;
          }
          double L[10], Linv[kNB], z[kNB];
#pragma unroll
          for (int c = 0; c < kNB; ++c) {
            double dsum = Sm[tri(c, c)];
#pragma unroll
            for (int m = 0; m < c; ++m) dsum = fma(-L[tri(c, m)], L[tri(c, m)], dsum);
            const double inv = rsqrt_refined(dsum);
            Linv[c] = ENDS ? inv * rs[c] : inv;
#pragma unroll
            for (int r = c + 1; r < kNB; ++r) {
              double t = Sm[tri(r, c)];
#pragma unroll
              for (int m = 0; m < c; ++m) t = fma(-L[tri(r, m)], L[tri(c, m)], t);
              L[tri(r, c)] = t * inv;
            }
          }
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
            double t = y[r];
#pragma unroll
            for (int m = 0; m < r; ++m) t = fma(-L[tri(r, m)], z[m], t);
            z[r] = t * Linv[r];
          }
          double* rec = rec0 + (size_t)(ENDS ? i : i - 1) * kQdRec * kQdPaths + pl;
          if (dim == 0) {
            rec[(kQdL + 0) * kQdPaths] = L[tri(1, 0)];
            rec[(kQdL + 1) * kQdPaths] = L[tri(2, 0)];
            rec[(kQdL + 2) * kQdPaths] = L[tri(2, 1)];
            rec[(kQdL + 3) * kQdPaths] = L[tri(3, 0)];
            rec[(kQdL + 4) * kQdPaths] = L[tri(3, 1)];
            rec[(kQdL + 5) * kQdPaths] = L[tri(3, 2)];
#pragma unroll
            for (int r = 0; r < kNB; ++r) rec[(kQdLinv + r) * kQdPaths] = Linv[r];
          }
#pragma unroll
          for (int r = 0; r < kNB; ++r) rec[(kQdZ + r * kD + dim) * kQdPaths] = z[r];
          // W = L^-1 E, then the Schur complement and right-hand side of vertex i + 1 (the last vertex: only when it has unknowns)
          if (i < S - 1 || (ENDS && fm_last != 0u)) {
            double W[kNB][kNB];
#pragma unroll
            for (int c = 0; c < kNB; ++c)
#pragma unroll
              for (int r = 0; r < kNB; ++r) {
                double t = cCpl[r][c] * p2[r + c + 2];
#pragma unroll
                for (int m = 0; m < r; ++m) t = fma(-L[tri(r, m)], W[m][c], t);
                W[r][c] = t * Linv[r];
              }
#pragma unroll
            for (int r = 0; r < kNB; ++r) {
#pragma unroll
              for (int c = 0; c <= r; ++c) {
                double t = cFar[tri(r, c)] * p2[r + c + 2];
#pragma unroll
                for (int m = 0; m < kNB; ++m) t = fma(-W[m][r], W[m][c], t);
                Sm[tri(r, c)] = t;
              }
              double t = -((cF[r] * p2[r + 1]) * dp);
#pragma unroll
              for (int m = 0; m < kNB; ++m) t = fma(-W[m][r], z[m], t);
              y[r] = t;
            }
          }
        }
        if (any_moving && i == 0) {  // vertex 1's right-hand side: - sum_c E[c][r] T^(r+c+2-2d) f_c
#pragma unroll
          for (int r = 0; r < kNB; ++r)
#pragma unroll
            for (int c = 0; c < kNB; ++c) y[r] = fma(-(cCpl[c][r] * p2[r + c + 2]), f0[c], y[r]);
        }
        if (ENDS && i == S - 1 && fm_last != 0u) {
          // the end vertex has unknowns: its block (the far part of the last segment, less what vertex S - 1 took) is complete
#pragma unroll
          for (int r = 0; r < kNB; ++r)
#pragma unroll
            for (int c = 0; c <= r; ++c)
              if (!((fm_last >> r) & 1u) || !((fm_last >> c) & 1u)) Sm[tri(r, c)] = (r == c) ? 1.0 : 0.0;
          double L[10], Linv[kNB], z[kNB];
#pragma unroll
          for (int c = 0; c < kNB; ++c) {
            double dsum = Sm[tri(c, c)];
#pragma unroll
            for (int m = 0; m < c; ++m) dsum = fma(-L[tri(c, m)], L[tri(c, m)], dsum);
            const double inv = rsqrt_refined(dsum);
            Linv[c] = ((fm_last >> c) & 1u) ? inv : 0.0;
#pragma unroll
            for (int r = c + 1; r < kNB; ++r) {
              double t = Sm[tri(r, c)];
#pragma unroll
              for (int m = 0; m < c; ++m) t = fma(-L[tri(r, m)], L[tri(c, m)], t);
              L[tri(r, c)] = t * inv;
            }
          }
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
            double t = y[r];
#pragma unroll
            for (int m = 0; m < r; ++m) t = fma(-L[tri(r, m)], z[m], t);
            z[r] = t * Linv[r];
          }
          double* rec = rec0 + (size_t)S * kQdRec * kQdPaths + pl;
          if (dim == 0) {
            rec[(kQdL + 0) * kQdPaths] = L[tri(1, 0)];
            rec[(kQdL + 1) * kQdPaths] = L[tri(2, 0)];
            rec[(kQdL + 2) * kQdPaths] = L[tri(2, 1)];
            rec[(kQdL + 3) * kQdPaths] = L[tri(3, 0)];
            rec[(kQdL + 4) * kQdPaths] = L[tri(3, 1)];
            rec[(kQdL + 5) * kQdPaths] = L[tri(3, 2)];
#pragma unroll
            for (int r = 0; r < kNB; ++r) rec[(kQdLinv + r) * kQdPaths] = Linv[r];
          }
#pragma unroll
          for (int r = 0; r < kNB; ++r) rec[(kQdZ + r * kD + dim) * kQdPaths] = z[r];
        }
      }
      p_cur = p_nxt;
      p_nxt = p_a2;
      p_a2 = p_a3;
      p_a3 = p_a4;
    }
    wave_lds_barrier();  // (lane 0 of a quad wrote L and W for the other three)
    // ---- backward: x_v = L^-T (z - W x_{v+1}); coefficients and cost of segment v from x_v, x_{v+1}
    double xn[kNB] = {0.0, 0.0, 0.0, 0.0};  // the last vertex is fully constrained (ENDS: or solved below, when it has unknowns)
    // (positions again, requested three vertices ahead of their use; a path shorter than the wavefront's longest joins late.
    // Keeping a copy of the positions in LDS instead -- no global load in this loop, so no s_waitcnt vmcnt(0) in front of
    // every step's stores -- was measured in round 5: no change at 65536 x 10, and the 5.6 KB it adds per wavefront cost
    // the grouped launch its fifth wavefront per CU: HISTORY.md)
    auto posb = [&](int v) { return (active && v >= 0 && v <= S) ? pv[(size_t)v * pstride] : 0.0; };
    double p_end = posb(S), p_b0 = posb(Smx - 1), p_b1 = posb(Smx - 2), p_b2 = posb(Smx - 3);
    for (int v = Smx - 1; v >= 0; --v) {
      const bool on = active && v < S;
      double x[kNB] = {0.0, 0.0, 0.0, 0.0};
      const double p_start = p_b0;
      p_b0 = p_b1;
      p_b1 = p_b2;
      p_b2 = posb(v - 3);
      if (ENDS && active && v == S - 1 && fm_last != 0u) {  // x_S = L^-T z of the end vertex (zero in its constrained slots)
        const double* rec = rec0 + (size_t)S * kQdRec * kQdPaths + pl;
        const double l10 = rec[(kQdL + 0) * kQdPaths], l20 = rec[(kQdL + 1) * kQdPaths], l21 = rec[(kQdL + 2) * kQdPaths],
                     l30 = rec[(kQdL + 3) * kQdPaths], l31 = rec[(kQdL + 4) * kQdPaths], l32 = rec[(kQdL + 5) * kQdPaths];
        const double i0 = rec[(kQdLinv + 0) * kQdPaths], i1 = rec[(kQdLinv + 1) * kQdPaths], i2 = rec[(kQdLinv + 2) * kQdPaths],
                     i3 = rec[(kQdLinv + 3) * kQdPaths];
        double t[kNB];
#pragma unroll
        for (int r = 0; r < kNB; ++r) t[r] = rec[(kQdZ + r * kD + dim) * kQdPaths];
        xn[3] = t[3] * i3;
        xn[2] = fma(-l32, xn[3], t[2]) * i2;
        xn[1] = fma(-l31, xn[3], fma(-l21, xn[2], t[1])) * i1;
        xn[0] = fma(-l30, xn[3], fma(-l20, xn[2], fma(-l10, xn[1], t[0]))) * i0;
      }
      if (on && (v >= 1 || (ENDS && fm_first != 0u))) {
        const double* rec = rec0 + (size_t)(ENDS ? v : v - 1) * kQdRec * kQdPaths + pl;
        double t[kNB];
#pragma unroll
        for (int r = 0; r < kNB; ++r) t[r] = rec[(kQdZ + r * kD + dim) * kQdPaths];
        const double l10 = rec[(kQdL + 0) * kQdPaths], l20 = rec[(kQdL + 1) * kQdPaths], l21 = rec[(kQdL + 2) * kQdPaths],
                     l30 = rec[(kQdL + 3) * kQdPaths], l31 = rec[(kQdL + 4) * kQdPaths], l32 = rec[(kQdL + 5) * kQdPaths];
        const double i0 = rec[(kQdLinv + 0) * kQdPaths], i1 = rec[(kQdLinv + 1) * kQdPaths], i2 = rec[(kQdLinv + 2) * kQdPaths],
                     i3 = rec[(kQdLinv + 3) * kQdPaths];
        // t = z - W x_{v+1},  W x = L^-1 (E x),  E[r][c] = HBAR[1+r][6+c] T_v^(r+c+2-2d)  (x_S = 0 unless the end vertex has unknowns)
        if (v < S - 1 || (ENDS && fm_last != 0u)) {
          double pw[9];
          quad_powers(tbuf[v * kQdPaths + pl], d1, d2, d4, pw);
          double u[kNB];
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
            u[r] = 0.0;
#pragma unroll
            for (int c = 0; c < kNB; ++c) u[r] = fma(cCpl[r][c] * pw[r + c + 2], xn[c], u[r]);
          }
          const double w0 = u[0] * i0;
          const double w1 = fma(-l10, w0, u[1]) * i1;
          const double w2 = fma(-l21, w1, fma(-l20, w0, u[2])) * i2;
          const double w3 = fma(-l32, w2, fma(-l31, w1, fma(-l30, w0, u[3]))) * i3;
          t[0] -= w0;
          t[1] -= w1;
          t[2] -= w2;
          t[3] -= w3;
        }
        x[3] = t[3] * i3;
        x[2] = fma(-l32, x[3], t[2]) * i2;
        x[1] = fma(-l31, x[3], fma(-l21, x[2], t[1])) * i1;
        x[0] = fma(-l30, x[3], fma(-l20, x[2], fma(-l10, x[1], t[0]))) * i0;
      }
      if (any_moving && v == 0 && active && moving_path) {  // the start vertex's constrained derivative values
        const double* vrow0 = vals + (size_t)pr.v0 * kHalf * kD + dim;
#pragma unroll
        for (int r = 0; r < kNB; ++r) {
          const double fr = vrow0[(r + 1) * kD];
          x[r] += (!ENDS || !((fm_first >> r) & 1u)) ? fr : 0.0;
        }
      }
      if (on) {
        const double T = tbuf[v * kQdPaths + pl];
        // c_k = T^-k sum_j ABAR_INV[k][j] T^(j%5) d_j ; cb_k = c_k T^k is what the cost needs
        const double dv[kN] = {p_start, x[0], x[1], x[2], x[3], p_end, xn[0], xn[1], xn[2], xn[3]};
        double w[kHalf];
        w[0] = 1.0;
#pragma unroll
        for (int k = 1; k < kHalf; ++k) w[k] = w[k - 1] * T;
        double db[kN], cb[kN], c[kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) db[j] = dv[j] * w[j % kHalf];
        const double ti = 1.0 / T;
        double tik = 1.0;
#pragma unroll
        for (int k = 0; k < kN; ++k) {
          double s = 0.0;
          if (k < kHalf) {
            s = c_abar_inv[k][k] * db[k];  // the upper half of ABAR_INV is diag(1/k!)
          } else {
#pragma unroll
            for (int j = 0; j < kN; ++j) s += c_abar_inv[k][j] * db[j];
          }
          cb[k] = s;
          c[k] = s * tik;
          tik *= ti;
        }
        double p2[9];
        quad_powers(T, d1, d2, d4, p2);  // p2[0] = T^(1 - 2d)
        my_cost = fma(cost_quadratic_form_d(d, cb), p2[0], my_cost);
        // the coefficients leave as five 16-byte pieces per lane (a lane owns 80 consecutive bytes).  Staging them through
        // the LDS of the consumed vertex records so that 16 lanes store 256 consecutive bytes of one path was built and
        // measured in round 5: 65536 x 10 129 -> 156 us -- the LDS round trip and its two wavefront syncs per step cost a
        // lone wavefront more than the 4x fewer write requests return (HISTORY.md)
        double2* out = reinterpret_cast<double2*>(coeffs + ((size_t)(pr.s0 + v) * kD + dim) * kN);
#pragma unroll
        for (int k = 0; k < kN; k += 2) store_coeff_pair(out + k / 2, c[k], c[k + 1]);
      }
#pragma unroll
      for (int r = 0; r < kNB; ++r) xn[r] = x[r];
      if (on) p_end = p_start;
    }
  } else if (active) {
    // ---- any other constraint pattern: the general masked step, factors in the plan's global workspace
    bool pok = true;
    BlockSource none{nullptr, nullptr, 0, 0};
    // (the times of this path, contiguous: the scaled ones were written to seg_times_out above, by this quad)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const double* times = (scaling ? tail.seg_times_out : seg_times) + pr.s0;
    my_cost = solve_path<1, true>(mask, vals, pr.v0, S, d, times, dim, none, ws, (size_t)b.n_paths * 4,
                                  (unsigned)q * 4u + (unsigned)dim, coeffs + (size_t)pr.s0 * kD * kN, pok);
  }
  my_cost = quad_sum(my_cost);
  if (active && dim == 0) {
    if (cost) cost[pr.p] = my_cost;
    if (status) {
      int st = merge_status(path_pos_ok, status_in, pr.p);
      if (tail.sum_t0 != nullptr && st > 0 && t_sum > MRS_TG_RUNAWAY_TIME_FACTOR * tail.sum_t0[pr.p]) st = MRS_TG_STATUS_ROUNDOFF_LIMITED;
      status[pr.p] = st;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The TWO-SIDED variant for launches that leave SIMDs idle (round 6).  A dispatch of 10240 paths is 640 quad wavefronts for
// 1024 SIMDs, each walking the chain of S - 1 vertices forward and back with its latencies exposed (VALU issue 19.7 %, wait
// share 45 %: profiles/round5_pmc_sq_solve_quad_group.json).  Here EIGHT lanes own a path -- side x dimension -- and a
// wavefront holds 8 paths: side 0 eliminates vertices 1 .. m - 1 from the start, side 1 eliminates S - 1 .. m + 1 from the
// end, the two meet at the middle vertex m = (S + 1) / 2: twice the wavefronts, half the dependent chain, the same LDS per CU.
//
// Side 1 runs the SAME instructions on the time-reversed path.  Reversing time maps a min-derivative problem onto itself:
// p~(t) = p(T - t) has derivatives (-1)^k p^(k) at the vertices, the cost is unchanged, and the unit-time constants are those
// of the forward problem.  So side 1 sees local vertex v = original vertex S - v, local segment i = original segment
// S - 1 - i, and its unknowns are the original ones with the odd derivatives negated (x~ = D x, D = diag(-1, +1, -1, +1) over
// the slots velocity .. snap).  At the join each side adds the other's Schur complement and right-hand side of the middle
// vertex -- D S D and D y, exact sign flips -- and both solve the same 4 x 4 system (bit-identical up to those signs); then
// each substitutes back through its own half and forms the coefficients of its own segments in FORWARD orientation from the
// end-point derivatives (side 1: start and end swapped, odd derivatives negated back).
// Plain paths only (position-only interior vertices, fully constrained ends; MOVING: a start vertex in motion, side 0's first
// step as in solve_quad_body); a wavefront with any other path takes the general masked step on the lanes of side 0.
// The results differ from solve_quad_body's in the last bits (another elimination order): same tolerances against the
// oracle's 113-bit route (tests/test_gpu_headline_kernel.py).
// Memory: every global load in the prologue, in one round; the position constraints, the times and the paths' indices wait in
// LDS; no register is carried across the loops that the compiler would spill ("What bounds the two-sided
// kernel": loads and stores share one in-order counter on gfx950, so a load or a scratch reload in the loops waits for the
// coefficient stores in flight).  Min-snap only (the launchers send nothing else).  Paths of up to 24 segments:
// the routing's only length rule is quad_kernel_applies, the four-lane record store within kQuadLdsBudget.
// (kDuoPaths, 8 paths per wavefront; kDuoXchgChunk, the chunk of the coefficient exchange; duo_lds_doubles: mrs_tg_solve_route.hpp)
// The chunk's 320 bytes change neither residency nor routing: the headline's 10 segments stay at eight wavefronts per CU (two per
// SIMD) within the CU's 160 KB, and at every length the four-lane kernel's record store -- the routing's only length rule,
// quad_kernel_applies -- is the larger of the two, so whatever that rule admits (24 segments today) fits kQuadLdsBudget here too.
static_assert(8 * duo_lds_doubles(10) * sizeof(double) <= 160 * 1024, "two-sided kernel at 10 segments: two wavefronts per SIMD");
static_assert(duo_lds_doubles(2) <= quad_lds_doubles(2) && duo_lds_doubles(24) <= quad_lds_doubles(24) &&
                  duo_lds_doubles(64) <= quad_lds_doubles(64),
              "(both grow linearly, the four-lane store faster: 432 against 248 doubles per segment)");

#ifdef MRS_TG_DUO_STAMPS  // experiment builds (build.py --variant): the shader clock at the phase boundaries of each wavefront
// slots 0 .. 13: the shader clock (s_memtime: one counter per XCD, not comparable across wavefronts of different XCDs); 14 and 15:
// the device-wide 100 MHz clock (s_memrealtime) at entry and behind the final wait -- first entry -> last exit of a dispatch
// in microseconds, and shader clocks per microsecond; 16: which dispatch wrote the row (the grouped kernel: its first batch's
// coefficient array), since the headline's two dispatches run side by side and share the rows
constexpr int kDuoStampSlots = 20;
__device__ unsigned long long g_duo_stamps[2048 * kDuoStampSlots];
#define DUO_STAMP(k) (duo_stamp[k] = __builtin_readcyclecounter())
#else
#define DUO_STAMP(k)
#endif

// The lane's index, formed where it is needed: under a register budget of three wavefronts per SIMD the compiler spills the
// values it derived from threadIdx.x in the prologue (the path's slot, the side, the dimension, LDS byte offsets) to scratch and
// reloads them inside the elimination loops -- vector-memory loads, which on gfx950 wait for the coefficient stores in flight
// (one counter for both).  Two instructions here instead; valid while all 64 lanes are enabled (wave-uniform control flow).
// (TAG: two statements with different tags are different instructions to the compiler, which therefore cannot merge the tails
// of two branches that end in them -- see duo_finish)
template <int TAG = 0>
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0 ; %1" : "=v"(l) : "i"(TAG));
  return l;
}

// the value of lane ^ 4 (the other side of the same path and dimension): ds_swizzle in bit-mask mode, no address register
__device__ __forceinline__ double xor4(double v) {
  constexpr int kSwap4 = (4 << 10) | 0x1F;  // and 0x1f, or 0, xor 4
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)u, kSwap4);
  const unsigned hi = (unsigned)__builtin_amdgcn_ds_swizzle((int)(unsigned)(u >> 32), kSwap4);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The epilogue of solve_duo_body: cost and status of the eight paths.  Written once per branch (TAG) instead of once behind
// both: behind the merge the compiler has to assume the general step's loads in flight and waits -- on gfx950 for all but the
// last few of the plain path's coefficient STORES as well (one counter), a store's round trip before the last two stores go out.
template <int TAG>
__device__ __forceinline__ void duo_finish(double my_cost, bool active, unsigned long long pos_bad, const int* pidx,
                                           double* __restrict__ cost, int32_t* __restrict__ status,
                                           const int32_t* __restrict__ status_in, const RowsTail& tail, double t_sum) {
  my_cost = quad_sum(my_cost);
  my_cost += xor4(my_cost);
  const int lane_late = lane_now<TAG + 1>();  // (the slot's address is formed HERE, not carried -- and spilled -- from the prologue)
  if (active && (lane_late & 7) == 0) {
    const bool path_pos_ok = ((pos_bad >> (lane_late & ~7)) & 0xFFull) == 0ull;
    const int p_out = pidx[lane_late >> 3];
    if (cost) cost[p_out] = my_cost;
    if (status) {
      int st = merge_status(path_pos_ok, status_in, p_out);
      if (tail.sum_t0 != nullptr && st > 0 && t_sum > MRS_TG_RUNAWAY_TIME_FACTOR * tail.sum_t0[p_out]) st = MRS_TG_STATUS_ROUNDOFF_LIMITED;
      status[p_out] = st;
      asm volatile("; epilogue %0" ::"i"(TAG));  // (keeps the two copies' tails apart: see above)
    }
  }
}

// THROUGH: the coefficient stores of the exchange road may be write-through stores (store_coeff_pair_through), `through` says
// whether this call's are (MRS_TG_DUO_STORE_THROUGH).  On for the grouped dispatch, whose coefficients nothing on the device
// reads next; off for the single launch: the sampling, the maxima or a second solve read its coefficients right behind it, and a
// written-through line does not stay in L2.
// LEAN: the batch is WHOLE-UNIFORM -- every path has the same even number of segments, at least 4, and the paths fill every
// wavefront (the launcher's rule: launch_solve_quad_group) -- with the uniform loops and the write-through stores on.  The same
// arithmetic in the same order (the lambdas and step bodies below are written once), without what serves partly filled or mixed
// wavefronts: no activity predicate, the path's place is arithmetic, the forward pass is the uniform loop alone, and the backward
// loop walks its LDS addresses by the per-lane stride, reads its positions unclamped and has the one store flavour -- exchange,
// then write-through -- that every step of an even length from 4 on takes.  The plainness test, the general step, cost and status
// are as in the other instantiation.
template <bool WP, bool MOVING = false, bool THROUGH = false, bool LEAN = false>
__device__ __forceinline__ void solve_duo_body(const BatchView& b, int d, const uint8_t* __restrict__ mask,
                                               const double* __restrict__ vals, const double* seg_times,
                                               double* __restrict__ coeffs, int32_t* __restrict__ status,
                                               double* __restrict__ cost, const int32_t* __restrict__ status_in, double* ws,
                                               const RowsTail& tail, int block, const double* __restrict__ pos_wp,
                                               bool uniform_loops, bool through = false) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x, pl = lane >> 3, side = (lane >> 2) & 1, dim = lane & 3, l8 = lane & 7;
  const int q = block * kDuoPaths + pl;
  static_assert(!LEAN || THROUGH, "the lean instantiation has the write-through flavour only");
  const bool active = LEAN || q < b.n_paths;
  const PathRef pr = LEAN ? PathRef{q, q * b.uniform_S, b.uniform_S, q * b.uniform_S + q} : path_at(b, active ? q : b.n_paths - 1);
  const int S = pr.S;
  const int Smax = b.max_segments;
  double* rec0 = lds;
  double* tbuf = lds + (size_t)(Smax > 1 ? Smax - 1 : 1) * kQdRec * kDuoPaths;  // [segment][path]
#ifdef MRS_TG_DUO_STAMPS
  unsigned long long duo_stamp[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  duo_stamp[14] = __builtin_amdgcn_s_memrealtime();
#endif
  DUO_STAMP(0);
  // ---- prologue: times (scaled, for the last solve of a Mellinger pipeline), plainness of the path, the position constraints
  // into LDS.  Every global load of the kernel is issued HERE, in one round (branch-free, indices clamped into the path): on
  // gfx950 loads and stores share one in-order counter (vmcnt), so a load inside the elimination loops makes each iteration
  // wait until the previous iteration's coefficient stores are acknowledged -- measured with the phase clocks of
  // -DMRS_TG_DUO_STAMPS: 3500 clocks per backward step, of which the arithmetic is a third (HISTORY.md, round 6).
  const bool scaling = tail.maxima != nullptr;
  double* pbuf = tbuf + (size_t)Smax * kDuoPaths;  // [vertex][dimension][path]
  int* pidx = reinterpret_cast<int*>(pbuf + (size_t)(Smax + 1) * kD * kDuoPaths);  // the paths' indices, for the epilogue: a register
  if (l8 == 0) pidx[pl] = pr.p;                                                     // held that long is spilled to scratch, and the
                                                                                    // reload is a vector-memory load (see above)
  DUO_STAMP(1);
  const double* pbase = WP ? pos_wp + (size_t)pr.v0 * kD : vals + (size_t)pr.v0 * kHalf * kD;
  constexpr int pstride = WP ? kD : kHalf * kD;
  const int n_pos = (S + 1) * kD;
  double t_sum = 0.0;
  bool ok = S >= 2, pos_ok = true;
  bool moving_path = false;
  auto mask_bits = [&](int v) {
    const uint8_t* mrow = mask + (size_t)(pr.v0 + v) * kHalf;
    unsigned fixed = 0;
#pragma unroll
    for (int k = 0; k < kHalf; ++k) fixed |= (mrow[k] != 0 ? 1u : 0u) << k;
    return fixed;
  };
  // the end vertices: even lanes of the eight read the start vertex's mask and constrained values, odd lanes the end vertex's
  // (lanes 0 and 1 decide)
  const int v_end = (l8 & 1) ? S : 0;
  const unsigned f_end = mask_bits(v_end);
  double av[kHalf * kD];
  // LEAN: the sixteen values of a path's end vertex spread over the four lanes of the eight that read it -- lane l8 has
  // derivative slot 1 + l8 / 2 -- and reduced below (nz is a sum of absolute values compared with zero: its order is free)
  const int k_end = 1 + (l8 >> 1);
  {
    const double* vrow = vals + (size_t)(pr.v0 + v_end) * kHalf * kD;
    if constexpr (LEAN) {
#pragma unroll
      for (int e = 0; e < kD; ++e) av[e] = fabs(vrow[k_end * kD + e]);
    } else {
#pragma unroll
      for (int e = kD; e < kHalf * kD; ++e) av[e] = fabs(vrow[e]);
    }
  }
  const int opt_st = (scaling && active) ? tail.opt_status[pr.p] : 0;
  auto trip = [&](int base) {               // sixteen segments and vertices of every path: two of each per lane
    const int ia = base + l8, ib = ia + 8;
    double Ta = seg_times[pr.s0 + min(ia, S - 1)], Tb = seg_times[pr.s0 + min(ib, S - 1)];
    const unsigned fa = mask_bits(min(ia, S)), fb = mask_bits(min(ib, S));
    double pe[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int ic = min(base * kD + k * 8 + l8, n_pos - 1);
      pe[k] = pbase[(size_t)(ic >> 2) * pstride + (ic & 3)];
    }
#ifdef MRS_TG_DUO_STAMPS
    if (base == 0) DUO_STAMP(13);
#endif
    if (active) {
      if (scaling) {  // scaleSegmentTimesToMeetConstraints (trajectory.cpp:625-657), then the solve at the scaled times
        if (ia < S) {
          if (opt_st != -2) Ta *= violation_scaling(tail.maxima + (size_t)(pr.s0 + ia) * 9, tail.limits + (size_t)pr.p * 9);
          tail.seg_times_out[pr.s0 + ia] = Ta;
        }
        if (ib < S) {
          if (opt_st != -2) Tb *= violation_scaling(tail.maxima + (size_t)(pr.s0 + ib) * 9, tail.limits + (size_t)pr.p * 9);
          tail.seg_times_out[pr.s0 + ib] = Tb;
        }
      }
      if (ia < S) {
        tbuf[ia * kDuoPaths + pl] = Ta;
        t_sum += Ta;
      }
      if (ib < S) {
        tbuf[ib * kDuoPaths + pl] = Tb;
        t_sum += Tb;
      }
      if (ia >= 1 && ia < S) {  // interior vertices: the position, nothing else
        ok = ok && fa == 0x1u;
        pos_ok = pos_ok && (fa & 1u);
      }
      if (ib < S) {
        ok = ok && fb == 0x1u;
        pos_ok = pos_ok && (fb & 1u);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int idx = base * kD + k * 8 + l8;
        if (idx < n_pos) pbuf[idx * kDuoPaths + pl] = pe[k];
      }
    }
  };
  // (the first trip is straight-line code -- all there is for batches of up to 15 segments: inside a loop the compiler has to
  // assume loads of the previous trip in flight and waits for the end vertices' values before it issues the positions' loads)
  trip(0);
  for (int base = 16; base <= Smax; base += 16) trip(base);
  double nz_end = 0.0;
  if constexpr (LEAN) {
    nz_end = ((f_end >> k_end) & 1u) ? (av[0] + av[1]) + (av[2] + av[3]) : 0.0;
    nz_end += dpp_move<0x4E>(nz_end);  // (lane ^ 2, then lane ^ 4: the four lanes of the eight with this lane's end vertex)
    nz_end += xor4(nz_end);
  }
  if (active && l8 < 2) {  // the end vertices: fully constrained, at rest (MOVING: the start vertex may be in motion)
    double nz = nz_end;
    if constexpr (!LEAN) {
#pragma unroll
      for (int k = 1; k < kHalf; ++k)
#pragma unroll
        for (int e = 0; e < kD; ++e) nz += ((f_end >> k) & 1u) ? av[k * kD + e] : 0.0;
    }
    if (MOVING && l8 == 0) {
      moving_path = nz != 0.0;
      nz = 0.0;
    }
    ok = ok && f_end == 0x1Fu && nz == 0.0;
    pos_ok = pos_ok && (f_end & 1u);
  }
  DUO_STAMP(2);
  t_sum = quad_sum(t_sum);
  t_sum += xor4(t_sum);
  const bool any_moving = MOVING && __ballot(active && moving_path) != 0ull;
  if (any_moving) moving_path = __shfl((int)moving_path, lane & ~7, 64) != 0 && side == 0;  // (vertex 0 was read by lane 0 of the eight)
  const bool plain_wave = __ballot(active && !ok) == 0ull;
  const unsigned long long pos_bad = __ballot(active && !pos_ok);
  // all eight paths present and of one length (MRS_TG_DUO_UNIFORM=0: no wavefront is treated as such)
  const bool uni_wave = LEAN || (uniform_loops && __ballot(active && S == __builtin_amdgcn_readfirstlane(S)) == ~0ull);
  wave_lds_barrier();
  DUO_STAMP(3);

  double my_cost = 0.0;
  if (plain_wave) {
    // (min-snap only: the launchers send no other objective order here -- with the order a constant the unit-time blocks are
    // literals instead of scalar loads the first step waits for, and one cost form is compiled instead of five)
    constexpr int kOrder = kHalf - 1;
    const double (*hb)[kN] = c_hbar[kOrder];
    double cNear[10], cCpl[kNB][kNB], cFar[10], cN[kNB], cF[kNB];
#pragma unroll
    for (int r = 0; r < kNB; ++r) {
#pragma unroll
      for (int c = 0; c <= r; ++c) {
        cNear[tri(r, c)] = hb[kSlot0 + r][kSlot0 + c];
        cFar[tri(r, c)] = hb[kHalf + kSlot0 + r][kHalf + kSlot0 + c];
      }
#pragma unroll
      for (int c = 0; c < kNB; ++c) cCpl[r][c] = hb[kSlot0 + r][kHalf + kSlot0 + c];
      cN[r] = hb[kSlot0 + r][0];
      cF[r] = hb[kHalf + kSlot0 + r][0];
    }
    constexpr bool d1 = (kOrder & 1) != 0, d2 = (kOrder & 2) != 0, d4 = (kOrder & 4) != 0;
    // this side's chain: local vertices 0 .. M (0: the path's end on this side, M: the middle vertex), local segments 0 .. M - 1
    const int m_mid = (S + 1) >> 1;
    // (wave-uniform trip count of both loops: the longest side the batch can hold -- a reduction over the wavefront's own paths
    // costs four cross-lane exchanges and their waits; ragged batches are sorted by length, a wavefront's paths differ by little)
    const int Mmx = (Smax + 1) >> 1;
    const int m_mid_ = m_mid;
    struct LaneIds { int pl, side, dim; };
    auto ids_now = [&]() {  // (see lane_now)
      const int l = lane_now();
      return LaneIds{l >> 3, (l >> 2) & 1, l & 3};
    };
    auto oseg = [&](int sd, int i) { return sd ? S - 1 - i : i; };   // original index of local segment i
    auto overt = [&](int sd, int v) { return sd ? S - v : v; };      // original index of local vertex v
    auto side_len = [&](int sd) { return sd ? S - m_mid_ : m_mid_; };
    auto pos = [&](const LaneIds& id, int v) {  // the position constraint of local vertex v (0 outside this side's chain)
      const int Ms = side_len(id.side);
      const int vc = min(max(v, 0), Ms);
      const double r = pbuf[(overt(id.side, vc) * kD + id.dim) * kDuoPaths + id.pl];
      return (active && v >= 0 && v <= Ms) ? r : 0.0;
    };
    // ---- forward: this side's block Cholesky towards the middle
    double Sm[10], y[kNB];
#pragma unroll
    for (int e = 0; e < 10; ++e) Sm[e] = 0.0;
#pragma unroll
    for (int r = 0; r < kNB; ++r) y[r] = 0.0;
    // The arithmetic of a forward step is written ONCE, in the two lambdas below, and used by two loops: the predicated one
    // (any mix of lengths in the wavefront, a partly filled wavefront) and the one for UNIFORM wavefronts (all eight paths
    // present, one length: every wavefront but the last of a batch of equal lengths, the runs of equal lengths of a sorted
    // ragged one).  Same operations in the same order on the same numbers: the same bits (tests/test_gpu_duo_bits.py).
    // (The backward loop has no uniform twin: its step as one straight block, or a second copy of it, makes the compiler park
    // some fifty of the step's constants in lanes of a VGPR and fetch them with v_readlane -- 410-450 instructions instead of
    // 366; and that loop was bound by its stores, not its instructions: DESIGN.md section 4.  That is about two copies in ONE
    // kernel: the LEAN instantiation holds the uniform form of the step alone -- 340 instructions, no v_readlane: item 6 there.)
    // local segment 0: the end vertex is fully constrained, the state moves to local vertex 1
    auto fwd_first = [&](const double (&p2)[9], double dp, const double (&f0)[kNB]) {
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) Sm[tri(r, c)] = cFar[tri(r, c)] * p2[r + c + 2];
        y[r] = -((cF[r] * p2[r + 1]) * dp);
      }
      if (any_moving) {  // local vertex 1's right-hand side: - sum_c E[c][r] T^(r+c+2-2d) f_c
#pragma unroll
        for (int r = 0; r < kNB; ++r)
#pragma unroll
          for (int c = 0; c < kNB; ++c) y[r] = fma(-(cCpl[c][r] * p2[r + c + 2]), f0[c], y[r]);
      }
    };
    // local vertex i >= 1: its block and right-hand side are complete with this segment's near part; rec: its record, at the
    // path's column
    auto fwd_interior = [&](const double (&p2)[9], double dp, double* rec, int dim_now) {
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) Sm[tri(r, c)] = fma(cNear[tri(r, c)], p2[r + c + 2], Sm[tri(r, c)]);
        y[r] = fma(-(cN[r] * p2[r + 1]), dp, y[r]);
      }
      double L[10], Linv[kNB], z[kNB];
#pragma unroll
      for (int c = 0; c < kNB; ++c) {
        double dsum = Sm[tri(c, c)];
#pragma unroll
        for (int mm = 0; mm < c; ++mm) dsum = fma(-L[tri(c, mm)], L[tri(c, mm)], dsum);
        const double inv = rsqrt_refined(dsum);
        Linv[c] = inv;
#pragma unroll
        for (int r = c + 1; r < kNB; ++r) {
          double t = Sm[tri(r, c)];
#pragma unroll
          for (int mm = 0; mm < c; ++mm) t = fma(-L[tri(r, mm)], L[tri(c, mm)], t);
          L[tri(r, c)] = t * inv;
        }
      }
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
        double t = y[r];
#pragma unroll
        for (int mm = 0; mm < r; ++mm) t = fma(-L[tri(r, mm)], z[mm], t);
        z[r] = t * Linv[r];
      }
      if (dim_now == 0) {
        rec[(kQdL + 0) * kDuoPaths] = L[tri(1, 0)];
        rec[(kQdL + 1) * kDuoPaths] = L[tri(2, 0)];
        rec[(kQdL + 2) * kDuoPaths] = L[tri(2, 1)];
        rec[(kQdL + 3) * kDuoPaths] = L[tri(3, 0)];
        rec[(kQdL + 4) * kDuoPaths] = L[tri(3, 1)];
        rec[(kQdL + 5) * kDuoPaths] = L[tri(3, 2)];
#pragma unroll
        for (int r = 0; r < kNB; ++r) rec[(kQdLinv + r) * kDuoPaths] = Linv[r];
      }
#pragma unroll
      for (int r = 0; r < kNB; ++r) rec[(kQdZ + r * kD + dim_now) * kDuoPaths] = z[r];
      // W = L^-1 E, then the Schur complement and right-hand side of local vertex i + 1 (always an unknown: the next one
      // of this side, or the middle vertex)
      double W[kNB][kNB];
#pragma unroll
      for (int c = 0; c < kNB; ++c)
#pragma unroll
        for (int r = 0; r < kNB; ++r) {
          double t = cCpl[r][c] * p2[r + c + 2];
#pragma unroll
          for (int mm = 0; mm < r; ++mm) t = fma(-L[tri(r, mm)], W[mm][c], t);
          W[r][c] = t * Linv[r];
        }
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          double t = cFar[tri(r, c)] * p2[r + c + 2];
#pragma unroll
          for (int mm = 0; mm < kNB; ++mm) t = fma(-W[mm][r], W[mm][c], t);
          Sm[tri(r, c)] = t;
        }
        double t = -((cF[r] * p2[r + 1]) * dp);
#pragma unroll
        for (int mm = 0; mm < kNB; ++mm) t = fma(-W[mm][r], z[mm], t);
        y[r] = t;
      }
    };
    // the start vertex's constrained derivative values (MOVING, side 0 of a path that starts in motion)
    auto moving_values = [&](int dim_now, double (&f)[kNB]) {
      const double* vrow0 = vals + (size_t)pr.v0 * kHalf * kD + dim_now;
#pragma unroll
      for (int r = 0; r < kNB; ++r) f[r] = vrow0[(r + 1) * kD];
    };
    // uniform wavefronts: S_u segments on every path, side 0 eliminates M0 vertices, side 1 M1 (M0 - M1 is 0 or 1); the uniform
    // loop takes the M1 steps that both sides have, the predicated loop the step in between (and every step of other wavefronts)
    const int S_u = __builtin_amdgcn_readfirstlane(S);
    const int M0 = (S_u + 1) >> 1, M1 = S_u - M0;
    int i_lo = 0, i_hi = Mmx;
    double p_cur;
    if (uni_wave) {
      // no predicate, no clamp; the LDS addresses of times, positions and records walk by a per-lane stride: + on side 0,
      // - on side 1 (original index of local segment i: i | S - 1 - i, of local vertex v: v | S - v)
      const LaneIds id = ids_now();
      const int v1 = id.side ? S_u - 1 : 1;  // local vertex 1; on side 1 also local segment 0
      const int st = id.side ? -kDuoPaths : kDuoPaths, sp = st * kD, sr = st * kQdRec;
      const double* tp = tbuf + (id.side ? v1 : 0) * kDuoPaths + id.pl;
      const double* pp = pbuf + (v1 * kD + id.dim) * kDuoPaths + id.pl;
      double* rp = rec0 + (v1 - 1) * kQdRec * kDuoPaths + id.pl;
      p_cur = pbuf[((id.side ? S_u : 0) * kD + id.dim) * kDuoPaths + id.pl];
      DUO_STAMP(4);
      {
        const double T = *tp, p_nxt = *pp;
        double p2[9];
        quad_powers(T, d1, d2, d4, p2);
        double f0[kNB] = {0.0, 0.0, 0.0, 0.0};
        if (any_moving && moving_path) moving_values(id.dim, f0);  // (side 0 only: moving_path is false on side 1)
        fwd_first(p2, p_cur - p_nxt, f0);
        p_cur = p_nxt;
      }
      DUO_STAMP(5);
      for (int i = 1; i < M1; ++i) {
        tp += st;
        pp += sp;
        const double T = *tp, p_nxt = *pp;
        double p2[9];
        quad_powers(T, d1, d2, d4, p2);
        fwd_interior(p2, p_cur - p_nxt, rp, lane_now() & 3);
        rp += sr;
        p_cur = p_nxt;
#ifdef MRS_TG_DUO_STAMPS
        if (i == 1) DUO_STAMP(6);
#endif
      }
      i_lo = M1;
      i_hi = M0;
    } else {
      p_cur = pos(ids_now(), 0);
      DUO_STAMP(4);
    }
    if constexpr (!LEAN)  // (an even uniform length: both sides have every step, the uniform loop has taken them all)
    for (int i = i_lo; i < i_hi; ++i) {
      const LaneIds id = ids_now();
      const bool on = active && i < side_len(id.side);
      const double T = on ? tbuf[oseg(id.side, i) * kDuoPaths + id.pl] : 1.0;
      const double p_nxt = pos(id, i + 1);
      double p2[9];
      quad_powers(T, d1, d2, d4, p2);
      const double dp = p_cur - p_nxt;
      double f0[kNB] = {0.0, 0.0, 0.0, 0.0};
      if (any_moving && i == 0 && active && moving_path) moving_values(id.dim, f0);  // (side 0 only, as above)
      if (on) {
        if (i == 0) {
          fwd_first(p2, dp, f0);
        } else {
          fwd_interior(p2, dp, rec0 + (size_t)(overt(id.side, i) - 1) * kQdRec * kDuoPaths + id.pl, id.dim);
        }
      }
      p_cur = p_nxt;
#ifdef MRS_TG_DUO_STAMPS
      if (i == 0) DUO_STAMP(5);
      if (i == 1) DUO_STAMP(6);
#endif
    }
    DUO_STAMP(7);
    // ---- the join: the middle vertex's block and right-hand side are this side's part plus the other side's, which arrives in
    // the other orientation: D S D and D y with D = diag(-1, +1, -1, +1) -- exact sign flips, so both sides solve the same
    // system and x~ = D x bit for bit
    double xn[kNB];
    {
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
#pragma unroll
        for (int c = 0; c <= r; ++c) {
          const double other = xor4(Sm[tri(r, c)]);
          Sm[tri(r, c)] += ((r + c) & 1) ? -other : other;
        }
        const double oy = xor4(y[r]);
        y[r] += (r & 1) ? oy : -oy;   // slot r is derivative r + 1: odd derivatives (r = 0, 2) change sign
      }
      double L[10], Linv[kNB], z[kNB];
#pragma unroll
      for (int c = 0; c < kNB; ++c) {
        double dsum = Sm[tri(c, c)];
#pragma unroll
        for (int mm = 0; mm < c; ++mm) dsum = fma(-L[tri(c, mm)], L[tri(c, mm)], dsum);
        const double inv = rsqrt_refined(dsum);
        Linv[c] = inv;
#pragma unroll
        for (int r = c + 1; r < kNB; ++r) {
          double t = Sm[tri(r, c)];
#pragma unroll
          for (int mm = 0; mm < c; ++mm) t = fma(-L[tri(r, mm)], L[tri(c, mm)], t);
          L[tri(r, c)] = t * inv;
        }
      }
#pragma unroll
      for (int r = 0; r < kNB; ++r) {
        double t = y[r];
#pragma unroll
        for (int mm = 0; mm < r; ++mm) t = fma(-L[tri(r, mm)], z[mm], t);
        z[r] = t * Linv[r];
      }
      xn[3] = z[3] * Linv[3];
      xn[2] = fma(-L[tri(3, 2)], xn[3], z[2]) * Linv[2];
      xn[1] = fma(-L[tri(3, 1)], xn[3], fma(-L[tri(2, 1)], xn[2], z[1])) * Linv[1];
      xn[0] = fma(-L[tri(3, 0)], xn[3], fma(-L[tri(2, 0)], xn[2], fma(-L[tri(1, 0)], xn[1], z[0]))) * Linv[0];
    }
    wave_lds_barrier();  // (the forward loop's records -- L written by the lane of dimension 0 for the other three -- are read below)
    DUO_STAMP(8);
    // ---- backward through this side's half: x_v = L^-T (z - W x_{v+1}); coefficients and cost of local segment v
    double p_end;
    // LEAN: the places of local vertex v's record and position, of local segment v's time (doubles from the start of LDS) and
    // of its coefficients (bytes from the wavefront's first segment) walk by the per-lane stride, as the forward loop's do
    int at_rec = 0, at_pos = 0, at_time = 0;
    unsigned at_out = 0;
    const int v_top = LEAN ? M1 - 1 : Mmx - 1;
    if constexpr (LEAN) {
      const LaneIds id = ids_now();
      p_end = pbuf[(M0 * kD + id.dim) * kDuoPaths + id.pl];  // (the middle vertex: S / 2 from either end)
      const int ov = id.side ? S_u - v_top : v_top, os = id.side ? ov - 1 : ov;  // original vertex and segment of local v_top
      at_rec = (ov - 1) * kQdRec * kDuoPaths + id.pl;
      at_pos = (int)(pbuf - lds) + (ov * kD + id.dim) * kDuoPaths + id.pl;
      at_time = (int)(tbuf - lds) + os * kDuoPaths + id.pl;
      at_out = (unsigned)(((id.pl * S_u + os) * kD * kN + 2 * id.dim) * (int)sizeof(double));
    } else {
      const LaneIds id = ids_now();
      p_end = pos(id, side_len(id.side));
    }
    for (int v = v_top; v >= 0; --v) {
      const LaneIds id = ids_now();
      const int side = id.side, dim = id.dim, pl = id.pl;  // (this iteration's: see lane_now)
      const bool on = LEAN || (active && v < side_len(side));
      double x[kNB] = {0.0, 0.0, 0.0, 0.0};
      double p_start, T_now = 0.0;
      if constexpr (LEAN) {
        p_start = lds[at_pos];
        T_now = lds[at_time];
      } else {
        p_start = pos(id, v);
      }
      if (on && v >= 1) {
        const double* rec = LEAN ? lds + at_rec : rec0 + (size_t)(overt(side, v) - 1) * kQdRec * kDuoPaths + pl;
        double t[kNB];
#pragma unroll
        for (int r = 0; r < kNB; ++r) t[r] = rec[(kQdZ + r * kD + dim) * kDuoPaths];
        const double l10 = rec[(kQdL + 0) * kDuoPaths], l20 = rec[(kQdL + 1) * kDuoPaths], l21 = rec[(kQdL + 2) * kDuoPaths],
                     l30 = rec[(kQdL + 3) * kDuoPaths], l31 = rec[(kQdL + 4) * kDuoPaths], l32 = rec[(kQdL + 5) * kDuoPaths];
        const double i0 = rec[(kQdLinv + 0) * kDuoPaths], i1 = rec[(kQdLinv + 1) * kDuoPaths], i2 = rec[(kQdLinv + 2) * kDuoPaths],
                     i3 = rec[(kQdLinv + 3) * kDuoPaths];
        {  // t = z - W x_{v+1},  W x = L^-1 (E x)  (local vertex v + 1 is an unknown for every v <= M - 1)
          double pw[9];
          quad_powers(LEAN ? T_now : tbuf[oseg(side, v) * kDuoPaths + pl], d1, d2, d4, pw);
          double u[kNB];
#pragma unroll
          for (int r = 0; r < kNB; ++r) {
            u[r] = 0.0;
#pragma unroll
            for (int c = 0; c < kNB; ++c) u[r] = fma(cCpl[r][c] * pw[r + c + 2], xn[c], u[r]);
          }
          const double w0 = u[0] * i0;
          const double w1 = fma(-l10, w0, u[1]) * i1;
          const double w2 = fma(-l21, w1, fma(-l20, w0, u[2])) * i2;
          const double w3 = fma(-l32, w2, fma(-l31, w1, fma(-l30, w0, u[3]))) * i3;
          t[0] -= w0;
          t[1] -= w1;
          t[2] -= w2;
          t[3] -= w3;
        }
        x[3] = t[3] * i3;
        x[2] = fma(-l32, x[3], t[2]) * i2;
        x[1] = fma(-l31, x[3], fma(-l21, x[2], t[1])) * i1;
        x[0] = fma(-l30, x[3], fma(-l20, x[2], fma(-l10, x[1], t[0]))) * i0;
      }
      if (any_moving && v == 0 && active && moving_path) {  // the start vertex's constrained derivative values (side 0)
        const double* vrow0 = vals + (size_t)pr.v0 * kHalf * kD + dim;
#pragma unroll
        for (int r = 0; r < kNB; ++r) x[r] += vrow0[(r + 1) * kD];
      }
      if (on) {
        const double T = LEAN ? T_now : tbuf[oseg(side, v) * kDuoPaths + pl];
        // the segment's end-point derivatives in FORWARD orientation: side 0 as they are, side 1 with start and end swapped
        // and the odd derivatives negated back
        const double s1 = side ? -1.0 : 1.0;
        const double a0 = side ? p_end : p_start, b0 = side ? p_start : p_end;
        double da[kNB], dbv[kNB];
#pragma unroll
        for (int r = 0; r < kNB; ++r) {
          const double sg = (r & 1) ? 1.0 : s1;
          da[r] = (side ? xn[r] : x[r]) * sg;
          dbv[r] = (side ? x[r] : xn[r]) * sg;
        }
        const double dv[kN] = {a0, da[0], da[1], da[2], da[3], b0, dbv[0], dbv[1], dbv[2], dbv[3]};
        double w[kHalf];
        w[0] = 1.0;
#pragma unroll
        for (int k = 1; k < kHalf; ++k) w[k] = w[k - 1] * T;
        double db[kN], cb[kN], c[kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) db[j] = dv[j] * w[j % kHalf];
        const double ti = 1.0 / T;
        double tik = 1.0;
#pragma unroll
        for (int k = 0; k < kN; ++k) {
          double sacc = 0.0;
          if (k < kHalf) {
            sacc = c_abar_inv[k][k] * db[k];  // the upper half of ABAR_INV is diag(1/k!)
          } else {
#pragma unroll
            for (int j = 0; j < kN; ++j) sacc += c_abar_inv[k][j] * db[j];
          }
          cb[k] = sacc;
          c[k] = sacc * tik;
          tik *= ti;
        }
        double p2[9];
        quad_powers(T, d1, d2, d4, p2);  // p2[0] = T^(1 - 2d)
        my_cost = fma(cost_quadratic_form<kOrder>(cb), p2[0], my_cost);
        double2* out = LEAN ? nullptr : reinterpret_cast<double2*>(coeffs + ((size_t)(pr.s0 + oseg(side, v)) * kD + dim) * kN);
        // A lane owns 80 consecutive bytes of its segment's 320, so a store instruction of 16 bytes per lane writes 64 separate
        // pieces over 50-odd cache lines, and the kernel is bound by that: with the stores left out a wavefront lives 30.7 k
        // clocks instead of 45.1 k (profiles/round6_duo_phase_clocks.txt, "stores").  In a uniform wavefront the four lanes of a
        // segment exchange their pairs through LDS first, so that an instruction writes 64 consecutive bytes per segment: 16
        // half lines.  The exchange buffer is one chunk of 320 bytes per segment; a quad of lanes writes and reads its own chunk
        // only.  The chunks lie in the records this step and the steps before it have read -- the rows of vertices v .. S - v,
        // S - 2 max(v, 1) + 1 of them (the middle vertex's row, which nobody writes, among them) -- and the sixteenth has a place of
        // its own (duo_lds_doubles):
        //   * a step of both sides (v < M1) has sixteen segments; fifteen chunks need three rows, which every such step has from
        //     S = 4 on -- the first step of a side, which has exactly three, included;
        //   * the step in between of an odd length (v = M1, side 0 alone: the lanes of side 1 are masked off here) has eight
        //     segments, chunk = path, and exactly two dead rows, the row of vertex v and the middle vertex's: eight chunks fit.
        //     The rows side 1 still has to read (vertices S - M1 + 1 .. S - 1) lie behind the middle vertex's;
        //   * what is left stores separate 16-byte pieces as before, at two lengths only: the one step of S = 2 (one row) and
        //     step 0 of S = 3 (two rows for sixteen segments).
        // One wavefront, LDS in program order: this step's reads of its records (the rows of vertices v and S - v, above) precede
        // the writes below, the rows of later steps (vertices < v and > S - v) are not touched, and the sync that closes a step
        // stands between its reads of the buffer and the next step's writes, the sixteenth chunk's included.
        constexpr int kRowDoubles = kQdRec * kDuoPaths;
        constexpr int kXchgRowsBoth = ((2 * kDuoPaths - 1) * kDuoXchgChunk + kRowDoubles - 1) / kRowDoubles;  // three today
        static_assert(kDuoPaths * kDuoXchgChunk <= 2 * kRowDoubles, "the step of side 0 alone: eight chunks in two rows");
        static_assert(kD == 4 && kN % 2 == 0, "a row of four lanes writes 64 consecutive bytes: one pair per dimension");
#if defined(MRS_TG_DUO_STORE_EXPERIMENT) && MRS_TG_DUO_STORE_EXPERIMENT == 1
        // experiment build (WRONG results; profiles/round6_duo_phase_clocks.txt, "stores"): no coefficient store at all
#pragma unroll
        for (int k = 0; k < kN; k += 2) asm volatile("; keep %0 %1" ::"v"(c[k]), "v"(c[k + 1]));
        if (false)
#elif defined(MRS_TG_DUO_STORE_EXPERIMENT) && MRS_TG_DUO_STORE_EXPERIMENT == 2
        // experiment build (WRONG results; same place): the step's 5120 bytes as whole lines inside the wavefront's own output
        if (uni_wave) {
          double2* wbase = reinterpret_cast<double2*>(coeffs + (size_t)(pr.s0 - pl * S) * kD * kN) + (v * 5 * 64 + (pl * 8 + side * 4 + dim));
#pragma unroll
          for (int k = 0; k < kN; k += 2) store_coeff_pair(wbase + (k / 2) * 64, c[k], c[k + 1]);
        } else
#endif
        if (LEAN || (uni_wave && (v >= M1 || S_u - 2 * max(v, 1) + 1 >= kXchgRowsBoth))) {
          const int chunk = (LEAN || v < M1) ? pl * 2 + side : pl;
          double* xrows = rec0 + (size_t)max(v - 1, 0) * kRowDoubles + chunk * kDuoXchgChunk;
          double* xlast = lds + (duo_lds_doubles(Smax) - kDuoXchgChunk);
          double2* xbuf = reinterpret_cast<double2*>(chunk == 2 * kDuoPaths - 1 ? xlast : xrows);
#pragma unroll
          for (int k = 0; k < kN; k += 2) xbuf[dim * (kN / 2) + k / 2] = make_double2(c[k], c[k + 1]);
          wave_lds_barrier();
          double2* out4 = out - 4 * dim;  // (the segment's first pair + this lane's place in a row of four; LEAN: at_out)
          // (all five reads ahead of the stores and of the branch: the assembly statements keep their order, and an LDS read
          // placed between two of them would be waited for there)
          double2 piece[kN / 2];
#pragma unroll
          for (int t = 0; t < kN / 2; ++t) piece[t] = xbuf[4 * t + dim];
          if constexpr (LEAN) {
            const double* wave_out = coeffs + (size_t)block * (kDuoPaths * kD * kN) * S_u;  // (the wavefront's first segment)
            store_coeff_pair_through<0>(wave_out, at_out, piece[0]);
            store_coeff_pair_through<64>(wave_out, at_out, piece[1]);
            store_coeff_pair_through<128>(wave_out, at_out, piece[2]);
            store_coeff_pair_through<192>(wave_out, at_out, piece[3]);
            store_coeff_pair_through<256>(wave_out, at_out, piece[4]);
          } else if (THROUGH && through) {
            static_assert(kN / 2 == 5, "one statement per pair");
            store_coeff_pair_through<0>(out4, piece[0]);
            store_coeff_pair_through<64>(out4, piece[1]);
            store_coeff_pair_through<128>(out4, piece[2]);
            store_coeff_pair_through<192>(out4, piece[3]);
            store_coeff_pair_through<256>(out4, piece[4]);
          } else {
#pragma unroll
            for (int t = 0; t < kN / 2; ++t) store_coeff_pair(out4 + 4 * t, piece[t].x, piece[t].y);
          }
          wave_lds_barrier();  // (the next step's records are other rows; the buffer of the next step overlaps this one)
        } else {
#pragma unroll
          for (int k = 0; k < kN; k += 2) store_coeff_pair(out + k / 2, c[k], c[k + 1]);
        }
      }
      if (on) {  // (a side shorter than the wavefront's longest joins late: until then xn is the middle vertex's solution)
#pragma unroll
        for (int r = 0; r < kNB; ++r) xn[r] = x[r];
        p_end = p_start;
      }
      if constexpr (LEAN) {  // local vertex and segment v - 1: one back on side 0, one on on side 1
        const int st = side ? kDuoPaths : -kDuoPaths;
        at_rec += st * kQdRec;
        at_pos += st * kD;
        at_time += st;
        at_out += (unsigned)(st * (kD * kN * (int)sizeof(double) / kDuoPaths));
      }
#ifdef MRS_TG_DUO_STAMPS
      if (v == v_top) DUO_STAMP(9);
#endif
    }
    DUO_STAMP(10);
    duo_finish<0>(my_cost, active, pos_bad, pidx, cost, status, status_in, tail, t_sum);
  } else {
    if (active && side == 0) {
    // ---- any other constraint pattern: the general masked step on the four lanes of side 0, factors in the plan's workspace
    bool pok = true;
    BlockSource none{nullptr, nullptr, 0, 0};
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    const double* times = (scaling ? tail.seg_times_out : seg_times) + pr.s0;
    my_cost = solve_path<1, true>(mask, vals, pr.v0, S, d, times, dim, none, ws, (size_t)b.n_paths * 4,
                                  (unsigned)q * 4u + (unsigned)dim, coeffs + (size_t)pr.s0 * kD * kN, pok);
    }
    duo_finish<2>(my_cost, active, pos_bad, pidx, cost, status, status_in, tail, t_sum);
  }
#ifdef MRS_TG_DUO_STAMPS
  DUO_STAMP(11);
  __builtin_amdgcn_s_waitcnt(0);  // (every store acknowledged)
  DUO_STAMP(12);
  duo_stamp[15] = __builtin_amdgcn_s_memrealtime();
  if (const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x; lane == 0 && wg < 2048)
    for (int k = 0; k < 16; ++k) g_duo_stamps[wg * kDuoStampSlots + k] = duo_stamp[k];
#endif
}

#ifdef MRS_TG_DUO_STAMPS
extern "C" int mrs_tg_debug_duo_stamps(unsigned long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_duo_stamps), sizeof(unsigned long long) * 2048 * kDuoStampSlots);
}
#endif

template <bool WP>
__global__ __launch_bounds__(64, MRS_TG_QUAD_WAVES) void solve_duo_kernel(BatchView b, int d, const uint8_t* __restrict__ mask,
                                                       const double* __restrict__ vals, const double* seg_times,
                                                       double* __restrict__ coeffs, int32_t* __restrict__ status,
                                                       double* __restrict__ cost, const int32_t* __restrict__ status_in,
                                                       double* ws, RowsTail tail, int uniform_loops) {
  solve_duo_body<WP, true>(b, d, mask, vals, seg_times, coeffs, status, cost, status_in, ws, tail, (int)blockIdx.x, tail.pos_wp,
                           (uniform_loops & 1) != 0);
}

// several batches of ONE plan in one launch: the grid is (workgroups of a batch, batches) -- the batch's index is there at entry,
// so its pointers load beside the other kernel arguments (a division of a linear index by a loaded count was two dependent
// scalar trips before any input address was known); workgroups are dispatched x first: the linear order is batch by batch
template <bool WP, bool LEAN = false>
__global__ __launch_bounds__(64, MRS_TG_DUO_GROUP_WAVES) void solve_duo_group_kernel(BatchView b, int d, RowsGroup g, double* ws,
                                                                                    size_t ws_batch_doubles, int uniform_loops) {
  const int j = (int)blockIdx.y;
  solve_duo_body<WP, false, true, LEAN>(b, d, g.mask[j], g.vals[j], g.seg_times[j], g.coeffs[j], g.status[j], g.cost[j], nullptr,
                                        ws + (size_t)j * ws_batch_doubles, RowsTail(), (int)blockIdx.x, g.pos_wp[j],
                                        (uniform_loops & 1) != 0, (uniform_loops & 2) != 0);
#ifdef MRS_TG_DUO_STAMPS
  if (const unsigned wg = blockIdx.y * gridDim.x + blockIdx.x; threadIdx.x == 0 && wg < 2048)
    g_duo_stamps[wg * kDuoStampSlots + 16] = (unsigned long long)g.coeffs[0];
#endif
}

template <bool WP, bool ENDS = false>
__global__ __launch_bounds__(64, MRS_TG_QUAD_WAVES) void solve_quad_kernel(BatchView b, int d, const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ vals, const double* seg_times,
                                                        double* __restrict__ coeffs, int32_t* __restrict__ status,
                                                        double* __restrict__ cost, const int32_t* __restrict__ status_in,
                                                        double* ws, RowsTail tail) {
  solve_quad_body<WP, ENDS, true>(b, d, mask, vals, seg_times, coeffs, status, cost, status_in, ws, tail, (int)blockIdx.x, tail.pos_wp);
}

// several batches of ONE plan in one launch (as solve_rows_group_kernel): workgroups [j * blocks_per_batch, ...) solve batch j
// (ws: one factor store of ws_batch_doubles per batch, for wavefronts that take the general step)
// (WP: every batch of the group states that its positions are its waypoints)
template <bool WP, bool ENDS = false>
__global__ __launch_bounds__(64, MRS_TG_QUAD_GROUP_WAVES) void solve_quad_group_kernel(BatchView b, int d, RowsGroup g, double* ws, size_t ws_batch_doubles,
                                                              int blocks_per_batch) {
  const int j = __builtin_amdgcn_readfirstlane((int)blockIdx.x / blocks_per_batch);
  solve_quad_body<WP, ENDS>(b, d, g.mask[j], g.vals[j], g.seg_times[j], g.coeffs[j], g.status[j], g.cost[j], nullptr,
                            ws + (size_t)j * ws_batch_doubles, RowsTail(), (int)blockIdx.x - j * blocks_per_batch, g.pos_wp[j]);
}

// ---------------------------------------------------------------------------------------------
// launchers: what the route says (route_solve, mrs_tg_solve_route.hpp), enqueued

static_assert(duo_lds_doubles(24) * sizeof(double) <= kQuadLdsBudget, "the two-sided kernel at the longest routed length");

hipError_t launch_solve_quad(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream,
                             const RowsTail& tail) {
  RowsTail tail_k = tail;
  tail_k.pos_wp = op.pos_wp;
  if (route.family == SolveFamily::kDuo) {  // few wavefronts: eight lanes per path, the chain cut in the middle
    const auto duo = route.wp ? MRS_TG_KERNEL(solve_duo_kernel<true>) : MRS_TG_KERNEL(solve_duo_kernel<false>);
    if (route.raise_lds_to)
      if (hipError_t e = set_max_dynamic_lds(duo, route.raise_lds_to); e != hipSuccess) return e;
    MRS_TG_LAUNCH_TIMED(duo, dim3(route.grid_x), dim3(route.threads), route.lds_bytes, stream, b, route.derivative, op.mask, op.vals,
                        op.seg_times, op.coeffs, op.status, op.cost, op.status_in, op.ws, tail_k, route.loop_bits);
    return hipGetLastError();
  }
  const auto quad = route.ends ? (route.wp ? MRS_TG_KERNEL(solve_quad_kernel<true, true>) : MRS_TG_KERNEL(solve_quad_kernel<false, true>))
                               : (route.wp ? MRS_TG_KERNEL(solve_quad_kernel<true>) : MRS_TG_KERNEL(solve_quad_kernel<false>));
  if (route.raise_lds_to)
    if (hipError_t e = set_max_dynamic_lds(quad, route.raise_lds_to); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(quad, dim3(route.grid_x), dim3(route.threads), route.lds_bytes, stream, b, route.derivative, op.mask, op.vals,
                      op.seg_times, op.coeffs, op.status, op.cost, op.status_in, op.ws, tail_k);
  return hipGetLastError();
}

hipError_t launch_solve_quad_group(const BatchView& b, const SolveRoute& route, const RowsGroup& g, double* ws, hipStream_t stream) {
  if (g.n < 1 || g.n > kRowsGroupMax || g.n != route.group || !uses_factor_store(route)) return hipErrorInvalidValue;
  const size_t ws_batch_doubles = linear_workspace_doubles(b);
  if (route.family == SolveFamily::kDuo) {
    // The lean instantiation's name in the trace is the family's -- an interface -- unless MRS_TG_TRACE_INSTANTIATIONS asks
    const bool spell = route.lean && knob::trace_instantiations();
    const auto duo = route.lean ? (route.wp ? kernel_as(solve_duo_group_kernel<true, true>, spell ? "solve_duo_group_kernel<true, true>" : "solve_duo_group_kernel<true>")
                                            : kernel_as(solve_duo_group_kernel<false, true>, spell ? "solve_duo_group_kernel<false, true>" : "solve_duo_group_kernel<false>"))
                                : (route.wp ? MRS_TG_KERNEL(solve_duo_group_kernel<true>) : MRS_TG_KERNEL(solve_duo_group_kernel<false>));
    if (route.raise_lds_to)
      if (hipError_t e = set_max_dynamic_lds(duo, route.raise_lds_to); e != hipSuccess) return e;
    MRS_TG_LAUNCH_TIMED(duo, dim3(route.grid_x, route.grid_y), dim3(route.threads), route.lds_bytes, stream, b, route.derivative, g, ws,
                        ws_batch_doubles, route.loop_bits);
    return hipGetLastError();
  }
  const auto quad = route.ends ? (route.wp ? MRS_TG_KERNEL(solve_quad_group_kernel<true, true>) : MRS_TG_KERNEL(solve_quad_group_kernel<false, true>))
                               : (route.wp ? MRS_TG_KERNEL(solve_quad_group_kernel<true>) : MRS_TG_KERNEL(solve_quad_group_kernel<false>));
  if (route.raise_lds_to)
    if (hipError_t e = set_max_dynamic_lds(quad, route.raise_lds_to); e != hipSuccess) return e;
  MRS_TG_LAUNCH_TIMED(quad, dim3(route.grid_x), dim3(route.threads), route.lds_bytes, stream, b, route.derivative, g, ws, ws_batch_doubles,
                      route.blocks_per_batch);
  return hipGetLastError();
}

}  // namespace mrs_tg

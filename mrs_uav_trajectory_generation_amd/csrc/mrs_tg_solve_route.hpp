// mrs_tg_solve_route.hpp -- the route of a fixed-times solve: WHICH kernel a solve launches, with which instantiation, grid and
// LDS -- one value (SolveRoute), computed from a request (SolveRequest) and the batch's shape by one pure function, route_solve.
// No HIP call, no allocation; the knobs are read through mrs_tg_knobs.hpp and nowhere else.  The launchers (mrs_tg_rows.hip,
// mrs_tg_quad.hip, mrs_tg_tile.hip, mrs_tg_kernels.hip) enqueue what the route says and decide nothing.
// Host-checkable (plain C++17 without a HIP include; tests/host/solve_route_harness.cpp runs it on the CPU).
// Of BatchView the routing reads n_paths, max_segments and uniform_S only.
#pragma once

#include <cstddef>

#include "mrs_tg_batch.hpp"
#include "mrs_tg_hd.hpp"
#include "mrs_tg_knobs.hpp"
#include "mrs_tg_transfer.hpp"

namespace mrs_tg {

// ---- LDS footprints and budgets (the kernels lay their LDS out by these; their static_asserts stay next to them) ----
// The dynamic LDS of a launch: a workgroup cannot have more than a compute unit's 160 KB, and more than the 64 KB a launch may
// ask for by default needs the kernel's limit raised first (a driver call, so only then).
constexpr size_t kLdsPerWorkgroup = 160 * 1024, kLdsDefaultLimit = 64 * 1024;

// the sampling walk (mrs_tg_sampling.hpp)
constexpr int kSampleBuffer = 192;  // samples parked per flush.  1024 made the LDS block of a 10-segment path 13.5 KB (11 wavefronts
                                    // per CU); 192: 5.2 KB, 30 per CU -- 8192 x 10: 50 -> 40 us (scripts/tile_phases.hip), 1024 x 10 unchanged

// rows kernel (mrs_tg_rows.hip): the sizes of its vertex and segment records
constexpr int kRVtxRec = 88, kRSegRec = 10;
MRS_TG_HD constexpr int rows_path_doubles(int S) {
  const int base = (S + 1) * kRVtxRec + S * kRSegRec + S * kD;
  return base + (base & 1) + 2;  // 16-byte aligned records, paths of a wavefront off each other's banks
}
constexpr size_t kRowsLdsBudget = 144 * 1024;
// LDS of one wavefront: the records of its paths, and for a launch that samples the times and coefficients of those paths
// plus one sample buffer
constexpr size_t rows_lds_bytes(int Smax, int ppw, bool sampling, bool maxima = false) {
  size_t doubles = (size_t)ppw * rows_path_doubles(Smax);
  if (sampling || maxima) doubles += (size_t)ppw * (size_t)Smax * (kD * kN + 1) + kSampleBuffer + kSampleBuffer / 4 + 2;
  if (maxima) doubles += (size_t)Smax * 9 + 10;  // + the path's nine limits
  return doubles * sizeof(double);
}

// four- and eight-lane kernels (mrs_tg_quad.hip): record size and paths per wavefront
constexpr int kQdRec = 26;
constexpr int kQdPaths = 16;  // paths per wavefront
// ends: records for the two end vertices as well (solve_quad_body<WP, true>: end vertices with free slots are eliminated)
MRS_TG_HD constexpr size_t quad_lds_doubles(int Smax, bool ends = false) {
  return (size_t)(ends ? Smax + 1 : (Smax > 1 ? Smax - 1 : 1)) * kQdRec * kQdPaths + (size_t)Smax * kQdPaths  // records | times
         + (ends ? (size_t)(Smax + 1) * 2 : 0)  // ends: the free mask of every (vertex, path), one byte each
      ;
}
constexpr int kDuoPaths = 8;  // paths per wavefront
// the coefficient exchange of a uniform wavefront (solve_duo_body's backward loop): one chunk of 4 dimensions x 10 coefficients
// per (path, side); the last of the sixteen chunks has a place of its own behind the path indices, the others lie in record rows
constexpr int kDuoXchgChunk = kD * kN;  // doubles
MRS_TG_HD constexpr size_t duo_lds_doubles(int Smax) {
  return (size_t)(Smax > 1 ? Smax - 1 : 1) * kQdRec * kDuoPaths + (size_t)Smax * kDuoPaths +  // records | times
         (size_t)(Smax + 1) * kD * kDuoPaths + kDuoPaths / 2 +                                  // | position constraints | path indices
         kDuoXchgChunk;                                                                         // | the sixteenth exchange chunk
}
constexpr size_t kQuadLdsBudget = 80 * 1024;  // at least two wavefronts per CU

// tile kernel (mrs_tg_tile.hip): record sizes (what they hold: there), per-path stride and workgroup size
constexpr int kSegRec = 16 + 4;            // coupling block EM (as its consumer reads it), qf[dim]
constexpr int kVtxRec = 42 + 20 + 2 + 2;   // D[10] -> L[10] | W[16] | Y[4][4] -> z[4][4] | d[5][4] | free bits, flags | pad
constexpr int kHandOver = 10 + 16;         // per path: the backward direction's Schur update for the middle vertex
// Per-path LDS stride.  Both record sizes are multiples of 8 doubles, so the unpadded stride put every path of a
// tile on the same banks ((a/4) mod 32 for ds_read2_b64 / ds_write*): the 16-lane groups of phase B (two paths x two
// directions) then hit one bank with up to four distinct addresses.  A stride of 4 (mod 16) doubles shifts each
// path by 8 banks.
MRS_TG_HD constexpr int tile_path_doubles(int S) {
  const int base = S * kSegRec + (S + 1) * kVtxRec + kHandOver;
  return base + ((4 - base % 16) + 16) % 16;
}
constexpr int kTileThreads = 256;
constexpr size_t kTileLdsBudget = 144 * 1024;

// ---- the predicates, each written once ----
// one lane per unknown, no materialised blocks (mrs_tg_rows.hip): the fused linear solve of every path that fits its LDS record
// (MRS_TG_ROWS_KERNEL=0 falls back to the tile and lane kernels)
inline bool rows_kernel_applies(const BatchView& b, bool with_sampling = false) {
  return b.n_paths != 0 && knob::rows_kernel() && rows_lds_bytes(b.max_segments, 1, with_sampling) <= kRowsLdsBudget;
}
// sampling on the solve's launch pays while a wavefront holds one path (small batches: one launch and one staging pass
// less, 1024 x 10 nonlinear 138 -> 132 us); with two paths per wavefront the walks of the two run one after the other and
// the separate sampler (one wavefront per path) is faster (8192 x 10: 483 vs 548 us)
inline bool rows_tail_sampling_pays(const BatchView& b) { return b.n_paths <= 2048 && rows_kernel_applies(b, true); }
// solve -> maxima -> scaling -> solve -> sampling of a pipeline in one launch of the rows kernel (small batches):
// up to one solving wavefront per SIMD (its helper shares the SIMD of another path's solver): 1024 x 10 pipeline 106.6 ->
// 101.0 us; at 2048 paths two solvers share every SIMD and the separate launches win (153 vs 169 us)
// (long paths: the separate launches again -- one 80-segment request 0.399 -> 0.379 ms, 64 x 80 0.706 -> 0.682, 48 / 49 segments
// on either side of a first threshold 0.182 / 0.176, equal at 30 segments; the results are the same bits either way,
// tests/test_gpu_pipeline_shortcuts.py)
inline bool rows_pipeline_applies(const BatchView& b) {
  return knob::rows_pipeline() && b.n_paths > 0 && b.n_paths <= 1024 && b.max_segments <= 32 &&
         rows_lds_bytes(b.max_segments, 1, true, true) <= kRowsLdsBudget;
}
// four lanes per path, factors in LDS (mrs_tg_quad.hip): launches that carry more paths than the rows kernel has wavefront
// slots for (paths_in_launch: of all batches a grouped launch carries).  The only length rule of the four- and eight-lane
// kernels: the four-lane record store within kQuadLdsBudget
inline bool quad_kernel_applies(const BatchView& b, long long paths_in_launch) {
  return b.n_paths != 0 && paths_in_launch >= knob::quad_min_paths() &&
         quad_lds_doubles(b.max_segments) * sizeof(double) <= kQuadLdsBudget;
}
// phase-split tile kernel (mrs_tg_tile.hip): small and medium batches whose per-path state fits in LDS.
// measured, 10 segments, one batch in flight, us per linear step / nonlinear pipeline (tile vs lane kernels):
//   blocks: 8192 paths 61 vs 83, 32768 271 vs 385, 65536 516 vs 572;
//   fused:  4096 316 vs 343, 8192 513 vs 537, 16384 840 vs 886, 32768 1498 vs 1639, 65536 2861 vs 2872
// -- since the vertex-accumulator layout (two workgroups per CU at eight paths per tile) the tile kernel wins at
// every size tried on uniform batches.  Ragged batches (3..30 segments: every tile is sized and looped for the
// longest path of the batch) cross over earlier: blocks 4096 paths 130 vs 163, 8192 225 vs 234, 16384 478 vs 349;
// fused 2048 779 vs 857, 4096 744 vs 736, 8192 1070 vs 960 (scripts/ragged_tile_sweep.py).
inline bool tile_kernel_applies(const BatchView& b, bool fused) {
  const long long max_paths = knob::tile_max_paths((b.uniform_S > 0) ? (1ll << 40) : (fused ? 4096 : 8192));
  if (b.n_paths == 0 || b.n_paths > max_paths) return false;
  // 32-bit byte offsets into the block buffers (load_H_blocks32)
  if (!fused && (unsigned long long)b.max_segments * 800ull * (unsigned long long)b.n_paths > 0xFFFFFFFFull) return false;
  return (size_t)tile_path_doubles(b.max_segments) * sizeof(double) <= kTileLdsBudget;
}
// The two-sided kernel takes a launch whose quad wavefronts (16 paths each) would leave SIMDs idle or barely covered: fewer than
// 1.25 per SIMD.  MRS_TG_DUO=0: never, =1: whenever the pattern allows (tuning / test knob, read at every call)
inline bool duo_pays(long long paths_in_launch, int compute_units) {
  if (const int forced = knob::duo_forced(); forced >= 0) return forced != 0;
  return (paths_in_launch + kQdPaths - 1) / kQdPaths < (long long)compute_units * 4 * 5 / 4;
}
// lane kernel: four lanes per path shorten the dependency chain ~4x but repeat the factorisation: worth it until the
// lanes of the 1-lane variant alone fill the machine
inline bool use_split_dims(int n_paths) { return n_paths <= 32768; }
// objective orders below snap leave jerk and / or snap free at the end vertices of a rest-to-rest path: the four-lane
// instantiation that eliminates such end vertices (two more records per path in LDS), while its LDS fits; MRS_TG_QUAD_ENDS=0:
// the general step for those paths, as until round 5
inline bool quad_ends_applies(const BatchView& b, int d, bool constrained_slots) {
  return knob::quad_ends() && (d < 4 || constrained_slots) && quad_lds_doubles(b.max_segments, true) * sizeof(double) <= kQuadLdsBudget;
}
// the two-sided kernels' `uniform_loops` argument: bit 0 MRS_TG_DUO_UNIFORM, bit 1 MRS_TG_DUO_STORE_THROUGH (the grouped kernel
// alone looks at it); both read at every call
inline int duo_loop_bits() { return (knob::duo_uniform() ? 1 : 0) | (knob::duo_store_through() ? 2 : 0); }
// the lean instantiation of the grouped two-sided kernel (solve_duo_body, LEAN): whole-uniform batches of an even length from 4
// on, every wavefront full, both loop knobs on
inline bool duo_lean_applies(const BatchView& b, int loop_bits) {
  return b.uniform_S >= 4 && b.uniform_S % 2 == 0 && b.n_paths % kDuoPaths == 0 && loop_bits == 3 && knob::duo_lean();
}

// ---- request and route ----
enum class SolveFamily {
  kNone,          // an empty batch: nothing is launched (grouped: also a batch that no grouped kernel takes)
  kDuo,           // eight lanes per path, the chain cut in the middle (solve_duo_kernel, solve_duo_group_kernel)
  kQuad,          // four lanes per path, factors in LDS (solve_quad_kernel, solve_quad_group_kernel)
  kRows,          // one lane per unknown (solve_rows_kernel, solve_rows_group_kernel)
  kRowsPipeline,  // solve -> maxima -> scaling -> solve (-> sampling) in one launch (solve_rows_pipeline_kernel)
  kTile,          // phase-split tiles (solve_tile_kernel)
  kLane,          // one or four lanes per path, state in registers and global memory (solve_linear_kernel)
};
// Where the solve stands.  The two stages put the same two rules in a different order, which shows only under
// MRS_TG_QUAD_MIN_PATHS <= 2048 (found and kept):
//   kFixedTimes: the sampling rides on the rows kernel (rows_tail_sampling_pays) BEFORE the four-lane kernel is asked;
//   kClosing (the solves that close a Mellinger pipeline): the four-lane kernel BEFORE the rows kernel's tail.
enum class SolveStage { kFixedTimes, kClosing };

struct SolveRequest {
  int derivative = 4;          // the objective order
  bool fused = true;           // false: from the materialised blocks
  bool factor_store = true;    // a global factor store is available (the four- and eight-lane kernels need one)
  int group = 0;               // batches of one plan in the launch; 0 = a single launch
  bool waypoints = false;      // the positions are the waypoints (MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS); grouped: of every batch
  RouteHints hints;
  int compute_units = 256;     // of the device, as the caller counts them (duo_pays)
  SolveStage stage = SolveStage::kFixedTimes;
  // what is wanted around the solve; the route says what it takes (scales, maxima_in_launch, sampling)
  bool scale_from_maxima = false;  // the feasibility scaling from given maxima, in front of the solve
  bool maxima_in_launch = false;   // solve, maxima of that trajectory, scaling and the solve again, in one launch
  bool sampling = false;           // the sampling behind the solve, if it can ride
  SolveFamily force = SolveFamily::kNone;  // kRows / kTile: that family whatever the size rules say (diagnostic programs)
};

struct SolveRoute {
  SolveFamily family = SolveFamily::kNone;
  int derivative = 4;
  int group = 0;
  // instantiation
  bool wp = false, ends = false, lean = false, with_tail = false, fused = true;
  int lanes_per_path = 0;      // lane kernel: 1 or 4
  int per_workgroup = 0;       // paths per wavefront (rows, quad, duo) / per tile / per 64-lane workgroup (lane)
  // launch
  unsigned grid_x = 0, grid_y = 1, threads = 64;
  int blocks_per_batch = 0;    // grouped: workgroups of one batch
  size_t lds_bytes = 0;
  size_t raise_lds_to = 0;     // the kernel's dynamic-LDS limit is raised to this first; 0: left alone
  int loop_bits = 0;           // two-sided kernels: duo_loop_bits
  // what of the request's surroundings the launch takes
  bool scales = false, maxima_in_launch = false, sampling = false;
};

// the four- and eight-lane kernels keep the factors of wavefronts that take the general masked step in a global store
inline bool uses_factor_store(const SolveRoute& r) { return r.family == SolveFamily::kDuo || r.family == SolveFamily::kQuad; }

namespace solve_route_detail {
inline unsigned cover(long long n, long long per) { return (unsigned)((n + per - 1) / per); }
inline size_t raise_over_default(size_t lds_bytes, size_t budget) { return lds_bytes > kLdsDefaultLimit ? budget : 0; }

inline void route_rows(SolveRoute& r, const BatchView& b, const SolveRequest& q) {
  r.family = SolveFamily::kRows;
  // one path per wavefront while that still leaves SIMDs idle (256 CUs x 4); two paths per wavefront otherwise -- and
  // when the caller says other batches share the device: at 255 VGPRs a SIMD holds two wavefronts, so 1024 one-path
  // wavefronts per launch let two launches run side by side, 512 two-path wavefronts four (1024 x 10, four streams:
  // 4.9 -> 4.1 us per step; alone on the device the two-path launch is 0.9 us slower).
  // Grouped: two paths per wavefront as soon as the launch carries more than one small batch: a host that groups launches
  // keeps several of them in flight (on alternating streams)
  int ppw = q.group > 0 ? ((long long)b.n_paths * q.group <= 1024 ? 1 : 2)
                        : ((b.n_paths <= 2048 && !(q.hints.shared_device && !r.sampling)) ? 1 : 2);
  if (knob::rows_ppw()) ppw = knob::rows_ppw();  // MRS_TG_ROWS_PPW=1|2
  if (rows_lds_bytes(b.max_segments, 2, r.sampling) > kRowsLdsBudget) ppw = 1;
  r.per_workgroup = ppw;
  r.lds_bytes = rows_lds_bytes(b.max_segments, ppw, r.sampling);
  r.raise_lds_to = raise_over_default(r.lds_bytes, kRowsLdsBudget);
  r.with_tail = r.sampling || r.scales;
  r.blocks_per_batch = (int)cover(b.n_paths, ppw);
  r.grid_x = (unsigned)r.blocks_per_batch * (unsigned)(q.group > 0 ? q.group : 1);
}

inline void route_rows_pipeline(SolveRoute& r, const BatchView& b) {
  r.family = SolveFamily::kRowsPipeline;  // two wavefronts per path
  r.per_workgroup = 1;
  r.with_tail = r.scales = r.maxima_in_launch = true;
  r.lds_bytes = rows_lds_bytes(b.max_segments, 1, true, true);
  r.raise_lds_to = raise_over_default(r.lds_bytes, kRowsLdsBudget);
  r.grid_x = (unsigned)b.n_paths;
  r.threads = 128;
}

inline void route_quad(SolveRoute& r, const BatchView& b, const SolveRequest& q, long long paths_in_launch) {
  r.wp = q.waypoints;
  r.ends = quad_ends_applies(b, q.derivative, q.hints.constrained_slots);
  const int groups = q.group > 0 ? q.group : 1;
  // few wavefronts: eight lanes per path (min-snap, fully constrained ends)
  if (!r.ends && !(q.derivative < 4) && duo_pays(paths_in_launch, q.compute_units)) {
    r.family = SolveFamily::kDuo;
    r.per_workgroup = kDuoPaths;
    r.loop_bits = duo_loop_bits();
    r.lean = q.group > 0 && duo_lean_applies(b, r.loop_bits);
    r.lds_bytes = duo_lds_doubles(b.max_segments) * sizeof(double);
    r.blocks_per_batch = (int)cover(b.n_paths, kDuoPaths);
    r.grid_x = (unsigned)r.blocks_per_batch;  // (grouped: x the batch's workgroups, y the batch)
    r.grid_y = (unsigned)groups;
  } else {
    r.family = SolveFamily::kQuad;
    r.per_workgroup = kQdPaths;
    r.lds_bytes = quad_lds_doubles(b.max_segments, r.ends) * sizeof(double);
    r.blocks_per_batch = (int)cover(b.n_paths, kQdPaths);
    r.grid_x = (unsigned)r.blocks_per_batch * (unsigned)groups;
  }
  r.raise_lds_to = raise_over_default(r.lds_bytes, kQuadLdsBudget);
  r.with_tail = r.scales;
}

inline void route_tile(SolveRoute& r, const BatchView& b) {
  r.family = SolveFamily::kTile;
  const size_t per_path = (size_t)tile_path_doubles(b.max_segments) * sizeof(double);
  int TP = (int)(kTileLdsBudget / per_path);
  if (TP > 8) TP = 8;  // phase B runs eight lanes per path inside wavefront 0
  // more, smaller tiles so that every CU gets work (256 CUs) and several tiles share a CU
  while (TP > 4 && (b.n_paths + TP - 1) / TP < 512) TP >>= 1;
  r.per_workgroup = TP;
  r.lds_bytes = per_path * (size_t)TP;
  r.raise_lds_to = kTileLdsBudget;
  r.grid_x = TP > 0 ? cover(b.n_paths, TP) : 0;
  r.threads = kTileThreads;
}

inline void route_lane(SolveRoute& r, const BatchView& b) {
  r.family = SolveFamily::kLane;
  // (the one-lane-per-path solve from materialised blocks -- 512 registers and 264 bytes of scratch per lane -- is gone: a
  // blocks solve of a batch the tile kernel does not take runs four lanes per path whatever its size)
  r.lanes_per_path = (use_split_dims(b.n_paths) || !r.fused) ? 4 : 1;
  r.per_workgroup = 64 / r.lanes_per_path;
  r.grid_x = cover((long long)b.n_paths * r.lanes_per_path, 64);
}
}  // namespace solve_route_detail

inline SolveRoute route_solve(const BatchView& b, const SolveRequest& q) {
  using namespace solve_route_detail;
  SolveRoute r;
  r.derivative = q.derivative;
  r.group = q.group;
  r.fused = q.fused;
  if (b.n_paths == 0) return r;
  const long long paths_in_launch = (long long)b.n_paths * (q.group > 0 ? q.group : 1);
  if (q.force == SolveFamily::kTile) {
    route_tile(r, b);
    return r;
  }
  if (q.force == SolveFamily::kRows) {
    r.scales = q.scale_from_maxima;
    r.sampling = q.sampling;
    if (q.maxima_in_launch) route_rows_pipeline(r, b);
    else route_rows(r, b, q);
    return r;
  }
  // saturated device: four (or eight) lanes per path, factors in LDS; no sampling on that launch
  const bool quad = q.fused && q.factor_store && quad_kernel_applies(b, paths_in_launch);
  if (q.group > 0) {  // grouped: the fixed-times default solve without a tail; kNone: no grouped kernel takes the batch
    if (quad) route_quad(r, b, q, paths_in_launch);
    else if (q.fused && rows_kernel_applies(b)) route_rows(r, b, q);
    return r;
  }
  const bool rides = q.fused && q.sampling && rows_tail_sampling_pays(b);
  if (q.maxima_in_launch && !quad && q.fused && rows_pipeline_applies(b)) {
    r.sampling = q.sampling;
    route_rows_pipeline(r, b);
  } else if (quad && !(q.stage == SolveStage::kFixedTimes && rides)) {
    r.scales = q.scale_from_maxima;
    route_quad(r, b, q, paths_in_launch);
  } else if (q.fused && rows_kernel_applies(b, rides)) {
    r.scales = q.scale_from_maxima;
    r.sampling = rides;
    route_rows(r, b, q);
  } else if (tile_kernel_applies(b, q.fused)) {
    route_tile(r, b);
  } else {
    route_lane(r, b);
  }
  return r;
}

}  // namespace mrs_tg

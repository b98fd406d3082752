// mrs_tg_nonlinear_route.hpp -- the route of a Mellinger outer loop: WHICH kernels launch_nonlinear enqueues, with which bins, grid
// and LDS -- one value (NonlinearRoute), computed by one pure function, route_nonlinear, from the host-only part of the plan
// (NonlinearHostPlan: the lane-group bins, built once per plan by nonlinear_host_plan), the batch's shape, the call's options and
// hints and the device's figures.  No HIP call, no allocation on the device; the knobs are read through mrs_tg_knobs.hpp and
// nowhere else.  The launchers (mrs_tg_nonlinear.hip, mrs_tg_wave.hip) map the route's enums to their kernels, enqueue what the
// route says and decide nothing.
// Host-checkable (plain C++17 without a HIP include; tests/host/nonlinear_route_harness.cpp runs it on the
// CPU).  Of BatchView the routing reads n_paths, max_segments and uniform_S only.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mrs_tg_batch.hpp"
#include "mrs_tg_hd.hpp"
#include "mrs_tg_knobs.hpp"
#include "mrs_tg_solve_route.hpp"
#include "mrs_tg_transfer.hpp"

// wavefronts per SIMD the lean kernels are compiled for (their __launch_bounds__) and the route counts residency by
#ifndef MRS_TG_LEAN_WAVES
#define MRS_TG_LEAN_WAVES 2
#endif

namespace mrs_tg {

// ---- LDS footprints (the kernels lay their LDS out by these: mrs_tg_sweep.hpp, mrs_tg_nonlinear.hip, mrs_tg_wave.hip; their
// static_asserts stay next to them) ----
constexpr int kLbfgsM = 5;
// what mrs_tg_sweep.hpp stages (what each record holds is said there):
constexpr int kVtxLds = 22;  // doubles per staged vertex: the 5 x 4 constrained values, 0 where free, then the free mask
constexpr int kSegLds = 38;  // doubles per staged segment record
constexpr int kStartExtraDim = 16 + 8 + 16;  // the moving-start extras in front of the segment records, per dimension
constexpr int kStartExtra = kD * kStartExtraDim;
constexpr int kBlockConsts = 36;  // the HBAR constants of the three 4 x 4 blocks of the one-sided sweeps
constexpr int kPsTable = 45;  // a direction table of the lean sweeps
constexpr int kPairState = 16;  // Sm[10], y[4], qf, red handed from the backward to the forward wavefront, per lane
// The optimiser's scalar state (f, alpha | neval, npairs, head, ret) is the same in every lane of a group; it is parked
// in LDS while the objective is evaluated, so that it does not occupy registers there (the kernel sits on its 256-VGPR
// cap and the compiler spilled exactly these to scratch memory, a global-memory round trip per reload).
constexpr int kTickState = 5;  // doubles: f, alpha, then six ints (neval, npairs, head, ret | guard tripped, spare)
constexpr int kLeanPub = 3 * 28;  // evaluate_lean_shared's hand-over area: three half-sweep states of 28 doubles
// behind it: the start vertex's constrained derivative values of a path that starts from a MOVING state (a replanning request
// in flight: velocity / acceleration / jerk of the first vertex constrained to non-zero values) -- [0] non-zero = there are
// such values, [2 + c * 4 + q] = derivative c + 1 of dimension q (zero where the slot is free)
constexpr int kLeanMoving = 18;
constexpr int kWaveMaxS = 12;  // 4 (S + 4) lanes <= 64: both directions of the two-sided evaluation in one wavefront
constexpr int kLeanTwoPassMaxS = 121;  // evaluate_lean_shared: 3 publishers + 61 other virtual lanes per pass, two passes

// per-group LDS block (doubles): x, g, xn, gn, dir [5*Sb], s[M][Sb], y[M][Sb], rho[M + 1], tick state, staged vertices
// [(Sb+1)*kVtxLds], moving-start extras [kStartExtra], staged segment records [Sb*kSegLds]
// extras: the moving-start area (only the one-dimension-per-lane kernels use it; in the four-dimensions-per-lane mapping
// of large batches many groups share a workgroup and 96 doubles each cost a workgroup per CU)
MRS_TG_HD constexpr int group_lds_doubles(int Sb, bool extras) {
  return (5 + 2 * kLbfgsM) * Sb + (kLbfgsM + 1) + kTickState + (Sb + 1) * kVtxLds + (extras ? kStartExtra : 0) + Sb * kSegLds;
}
// cost_gradient_kernel: x, g [2*Sb], staged vertices
MRS_TG_HD constexpr int gradient_lds_doubles(int Sb, bool extras) {
  return 2 * Sb + (Sb + 1) * kVtxLds + (extras ? kStartExtra : 0) + Sb * kSegLds;
}
MRS_TG_HD constexpr int lean_eval_doubles(int Sb) { return 4 * Sb + 4 * (Sb + 1) + kLeanPub + kLeanMoving; }  // dp, staging area, hand-over, moving start
// per-group LDS of the plain-path kernels and their staging
MRS_TG_HD constexpr int lean_group_doubles(int Sb) {
  return (5 + 2 * kLbfgsM) * Sb + (kLbfgsM + 1) + kTickState + lean_eval_doubles(Sb);
}

// ---- the bins ----
// Paths are sorted by segment count (longest first), so every lane-group class is a contiguous range of positions q.
struct NonlinearBin {
  int group;      // lanes per path: 4, 8, 16, 32 or 64
  int q_begin;    // first position of the bin
  int q_count;    // number of paths in the bin
  int max_S;      // largest segment count in the bin
  int min_S;      // smallest
};

// All bins of a plan run in ONE launch: blocks [block_begin, block_begin + n_blocks) of the grid belong to a
// bin (paths sorted longest first, so the long paths are dispatched first and the short ones fill the tail).
// A kernel argument: name, namespace and layout are part of the kernels' signatures.
constexpr int kMaxBins = 5;  // the five group widths; a launch whose bins do not fit the table is not made (route_nonlinear)
struct BinTable {
  int n;
  int group[kMaxBins], q_begin[kMaxBins], q_count[kMaxBins], max_S[kMaxBins], block_begin[kMaxBins];
};

// the host-only part of a plan (NonlinearPlan, mrs_tg_nonlinear.h, holds it next to its device blocks)
struct NonlinearHostPlan {
  std::vector<NonlinearBin> bins;
  std::vector<NonlinearBin> bins1;   // the one-lane-per-vector groups of a plan whose own choice is the dimension split (regroup_possible)
  bool regroup_possible = false;     // a call may take the lane-group kernels instead of the split kernel (route_nonlinear)
  // the plain-path outer loop's bins when EVERY path of four or more segments gets the lanes of the shared half sweeps
  // (G = pow2ceil(S + 4) instead of pow2ceil(S + 1): 5-7, 13-15 and 29-30 segments move to the next group width); chosen
  // by route_nonlinear while the launch is about as large as the device holds at once (see there)
  std::vector<NonlinearBin> wide_bins;
  int wide_blocks = 0;             // workgroups of a launch over wide_bins
  // objective orders below snap (free slots at the end vertices): every path of four or more segments in a group of at least
  // S + 4 lanes, for the shared half sweeps with free ends (optimize_lean_shared_ends_kernel); empty when a path is too long
  std::vector<NonlinearBin> ends_bins;
  int dim_split = 1;               // lanes per time vector in the outer loop: 1 (compact) or 4 (one per dimension)
};

// split the four dimensions over lanes while the batch is too small to fill the machine otherwise
inline int dim_split_for(int n_paths, int max_S) {
  if (const int forced = knob::dim_split_max_paths(); forced != knob::kUnset) return n_paths <= forced ? 4 : 1;  // tuning knob
  // One lane per dimension pays while a path's (S + 1) x 4 lanes fit ONE wavefront: from 16 segments on the split kernel
  // walks a path in several passes and the lean kernel's lane groups are 2-3x faster at every batch size (whole pipeline,
  // scripts/measure_configs.py uniform<P>x<S>, profiles/round5_dim_split_crossover.txt: 256 x 16 0.378 vs 0.168 ms,
  // 2048 x 30 1.290 vs 0.429 ms, 1024 ragged 3..30 0.681 vs 0.240 ms).
  if (max_S > 15) return 1;
  // measured cross-over against the lean kernel of large batches (scripts/ps_step.py with MRS_TG_DIM_SPLIT_MAX_PATHS=0):
  // outer-loop kernel 2048 paths 122 vs 143 us, 3072 paths 160 vs 150 us (10 segments); 13 segments: 1024 paths 0.152 vs
  // 0.168 ms, 2048 paths 0.220 vs 0.192 ms (whole pipeline)
  return n_paths <= (max_S > 12 ? 1536 : 2560) ? 4 : 1;
}

// A path with S segments uses a group of G = min(64, pow2ceil((S + 1) * ds)) lanes: lane k of the group evaluates the cost at the
// k-th perturbed time vector (k = 0: unperturbed), with ds lanes per vector
inline int group_for(int S, int ds) {
  int G = 4;
  while (G < (S + 1) * ds && G < 64) G <<= 1;
  return G;
}

// lanes per path when the long paths get the S + 4 lanes of the shared half sweeps: 13-15 and 29-30 segments move to the next
// group width.  (5-7 segments stay in groups of 8 and their one-sided sweeps: six steps against four do not pay for half
// the paths per wavefront -- 8192 x 6: 0.190 ms narrow, 0.197 ms wide; 65536 x 6: 0.861 vs 1.015 ms.)  These bins decide
// WHETHER a launch is small enough for wide groups (wide_blocks) and are what MRS_TG_LEAN_WIDE_ALL=0 launches; by default
// such a launch uses the bins of group_for_ends below (every path of two or more segments in S + 4 lanes: route_nonlinear)
inline int group_for_wide(int S) {
  int G = group_for(S, 1);
  if (S >= 13 && G < S + 4 && G < 64) G <<= 1;
  return G;
}

// lanes per path when EVERY path of MRS_TG_ENDS_MIN_SEGMENTS or more segments gets its S + 4 lanes (0: no group is wide enough).
// Two segments are enough for the shared half sweeps (one step per half); handing the 2- and 3-segment paths of a ragged
// batch to the sweeping kernel BEHIND the launch instead cost 8192 ragged paths 0.67 instead of 0.58 ms (d = 2).
inline int group_for_ends(int S) {
  if (S < knob::ends_min_segments()) return group_for(S, 1);
  if (S + 4 > 64) return S <= kLeanTwoPassMaxS ? 64 : 0;  // a wavefront per path, two passes of the shared evaluation
  int G = 8;
  while (G < S + 4) G <<= 1;
  return G;
}

// workgroups (one wavefront each) of a bin
inline int bin_blocks(const NonlinearBin& bin) { return (int)solve_route_detail::cover(bin.q_count, 64 / bin.group); }

template <class GroupFor>
inline void build_bins(std::vector<NonlinearBin>& bins, const std::vector<int32_t>& so, const std::vector<int32_t>& order,
                       GroupFor group_of) {
  bins.clear();
  const int P = (int)order.size();
  int q = 0;
  while (q < P) {
    const int p = order[q];
    const int S = so[p + 1] - so[p];
    NonlinearBin bin;
    bin.group = group_of(S);
    bin.q_begin = q;
    bin.max_S = S;  // sorted longest first: the first path of a bin is its longest
    int e = q;
    while (e < P && group_of(so[order[e] + 1] - so[order[e]]) == bin.group) ++e;
    bin.q_count = e - q;
    bin.min_S = so[order[e - 1] + 1] - so[order[e - 1]];  // ... and the last one its shortest
    bins.push_back(bin);
    q = e;
  }
}

// so: the batch's segment offsets [n_paths + 1] in the caller's path order; order: position -> path, longest first (stable)
inline NonlinearHostPlan nonlinear_host_plan(const std::vector<int32_t>& so, const std::vector<int32_t>& order) {
  NonlinearHostPlan nl;
  const int P = (int)order.size();
  const int max_S = P > 0 ? so[order[0] + 1] - so[order[0]] : 0;  // (sorted longest first)
  nl.dim_split = dim_split_for(P, max_S);
  const int ds = nl.dim_split;
  build_bins(nl.bins, so, order, [ds](int S) { return group_for(S, ds); });
  // The lane-group layouts as well where a CALL may prefer them to the plan's dimension split (route_nonlinear: 13-15
  // segments under an objective order below snap or with constrained slots / moving starts, whose paths the split kernel
  // hands to its general step): the plan is built before the options are known
  nl.regroup_possible = ds == 4 && max_S >= 13 && max_S <= 15;
  const bool groups = ds == 1 || nl.regroup_possible;
  if (nl.regroup_possible) build_bins(nl.bins1, so, order, [](int S) { return group_for(S, 1); });
  if (groups) {
    build_bins(nl.wide_bins, so, order, [](int S) { return group_for_wide(S); });
    for (const NonlinearBin& bin : nl.wide_bins) nl.wide_blocks += bin_blocks(bin);
  }
  if (groups && P > 0 && group_for_ends(max_S) != 0)
    build_bins(nl.ends_bins, so, order, [](int S) { return group_for_ends(S); });
  return nl;
}

// ---- the predicates and the launches' LDS, each written once ----
// Lean sweeps for plain paths (optimize_lean_kernel): two wavefronts per SIMD where the general sweeping kernel has one.
// Objective orders below snap leave slots free at the end vertices of a rest-to-rest path: optimize_lean_masked_kernel takes
// those (masked step at the two ends of the sweep), at one wavefront per SIMD -- 256 + 74 registers; forced to two it spills
// 96 and loses to the general kernel (8192 x 10 random-walk paths at d = 2: 429 vs 365 us; at one wavefront 332 us).
inline bool lean_applies(int dim_split) {
  if (const int forced = knob::lean_forced(); forced >= 0) return forced != 0;
  return dim_split == 1;
}
// one wavefront per path (mrs_tg_wave.hip): small batches (the call's dim_split == 4) whose longest path has at most kWaveMaxS
// segments; MRS_TG_WAVE_KERNEL=0 disables
inline bool wave_kernel_applies(const BatchView& b, int dim_split) {
  return knob::wave_kernel() && dim_split == 4 && b.n_paths > 0 && b.max_segments <= kWaveMaxS;
}
// a wavefront of a lean launch: its groups and the two direction tables
inline size_t lean_lds_bytes(const NonlinearBin& bin) {
  return ((size_t)(64 / bin.group) * lean_group_doubles(bin.max_S) + 2 * kPsTable) * sizeof(double);
}
// a wavefront of a sweeping launch: its groups (split: with the moving-start area) and the block constants
inline size_t sweep_lds_bytes(const NonlinearBin& bin, bool split) {
  return ((size_t)(64 / bin.group) * group_lds_doubles(bin.max_S, split) + kBlockConsts) * sizeof(double);
}
// optimize_careful_kernel, optimize_general_kernel: one listed path per workgroup of 64, sized for the batch's longest
inline size_t listed_lds_bytes(int max_S) { return ((size_t)group_lds_doubles(max_S, true) + kBlockConsts) * sizeof(double); }
// cost_gradient_kernel, launched bin by bin
inline size_t gradient_lds_bytes(const NonlinearBin& bin, bool split) {
  return ((size_t)(64 / bin.group) * gradient_lds_doubles(bin.max_S, split) + kBlockConsts) * sizeof(double);
}
// "as many paths per launch as a 2 GB factor store holds": the lanes of optimize_careful_kernel and optimize_general_kernel keep
// per_path_doubles each; at least 16 paths, at most `cap`
inline size_t factor_store_paths(size_t per_path_doubles, size_t cap) {
  return std::min(cap, std::max<size_t>((size_t)16, ((size_t)1 << 28) / per_path_doubles));
}

// the kernel's table of `bins`; returns the largest lds_of(bin) and leaves the workgroup count in *blocks
template <class LdsOf>
inline size_t fill_bin_table(BinTable& bt, const std::vector<NonlinearBin>& bins, LdsOf lds_of, int* blocks) {
  bt.n = (int)bins.size();
  size_t lds = 0;
  *blocks = 0;
  for (int i = 0; i < bt.n; ++i) {
    const NonlinearBin& bin = bins[i];
    bt.group[i] = bin.group;
    bt.q_begin[i] = bin.q_begin;
    bt.q_count[i] = bin.q_count;
    bt.max_S[i] = bin.max_S;
    bt.block_begin[i] = *blocks;
    *blocks += bin_blocks(bin);
    lds = std::max(lds, lds_of(bin));
  }
  return lds;
}

// ---- the route ----
// the instantiations of the outer loop a launcher chooses between (mrs_tg_nonlinear.hip maps each to its kernel, once)
enum class LeanKernel {
  kLean,               // one-sided sweeps, and the shared half sweeps wave by wave (optimize_lean_kernel)
  kLeanMasked,         // one-sided sweeps with the masked step at the two ends (optimize_lean_masked_kernel)
  kLeanShared,         // shared half sweeps only (optimize_lean_shared_kernel)
  kLeanSharedEnds,     // ... with free end slots (optimize_lean_shared_ends_kernel)
  kLeanSharedEndsLong, // ... two passes per wavefront (optimize_lean_shared_ends_long_kernel)
};
enum class SweepKernel {
  kWave,           // one wavefront per path (optimize_wave_kernel, mrs_tg_wave.hip)
  kSplit,          // one dimension per lane (optimize_split_kernel)
  kCompact,        // four dimensions per lane (optimize_compact_kernel<false>)
  kCompactMasked,  // ... with the masked step compiled in (optimize_compact_kernel<true>)
};

struct OuterLaunch {
  BinTable bins{};
  int blocks = 0;
  unsigned threads = 64;
  size_t lds_bytes = 0;
};

// what follows the outer loop: a reading of the closing solves' routes (NonlinearRoute::first_solve, final_solve)
enum class Closing {
  kRowsPipeline,  // solve -> maxima -> scaling -> solve (-> sampling) in one launch of the rows kernel
  kQuadTail,      // solve, maxima, then the scaling on the quad kernel's final solve (the caller's sampler follows)
  kRowsTail,      // solve, maxima, then scaling (and sampling) on the rows kernel's final solve
  kSeparate,      // solve, maxima, scaling, runaway test and final solve as launches of their own
};

struct NonlinearRoute {
  bool estimate_in_kernel = false;  // the outer-loop kernels compute the start point themselves (else: a launch in front of them)
  int dim_split = 1;                // of THIS call: 1 where it goes back from the plan's dimension split to lane groups
  // 1a. the lean kernel takes every plain path and flags the others for the sweeping kernel behind it
  bool lean = false;
  LeanKernel lean_kernel = LeanKernel::kLean;
  OuterLaunch lean_launch;
  bool queued = false;              // the launch holds what is resident; lane groups claim further paths from the plan's queue
  // 1b. the sweeping kernel: alone, or behind the lean kernel for the paths that one flagged
  SweepKernel sweep_kernel = SweepKernel::kWave;
  bool wave() const { return sweep_kernel == SweepKernel::kWave; }  // one wavefront per path: no bins, no dynamic LDS
  bool sweep_fits = true;           // false: more than five bins or more LDS than a workgroup can have -- the call fails there
  OuterLaunch sweep_launch;
  bool careful = false;             // 1c. the careful re-run follows
  bool general = false;             // 1d. the outer loop of the paths with a position-free vertex follows (and their solves below)
  bool certified_maxima = true;     // segment_maxima_scaling_kernel, else every entry searched (segment_maxima9_kernel)
  // the closing solves, routed as every fixed-times solve is (route_solve): the trajectory of the last evaluated point (not
  // launched where the final solve takes the maxima into its own launch), and the solve at the scaled times
  SolveRoute first_solve, final_solve;
  Closing closing() const {
    return final_solve.maxima_in_launch           ? Closing::kRowsPipeline
           : !final_solve.scales                  ? Closing::kSeparate
           : uses_factor_store(final_solve)       ? Closing::kQuadTail
                                                  : Closing::kRowsTail;
  }
  bool tail_samples() const { return final_solve.sampling; }  // the sampling rides on the closing launch
};

// nl: the plan's host part; hints: the call's (RouteHints, launch_nonlinear's argument); compute_units: of the current device;
// resident_blocks: workgroups of a queued lean launch, 0 = no queue.  The CALLER owns that rule: the library passes one figure for
// the whole process (MRS_TG_LEAN_RESIDENT_BLOCKS, else what the first device it asked holds: launch_nonlinear), a harness a number.
// closing: the request of the closing solves as solve_request fills it (objective order, hints, factor store, waypoints and the
// compute units the solve routes by); estimate: the search starts from the estimate; samples_wanted: the caller asked for samples
inline NonlinearRoute route_nonlinear(const NonlinearHostPlan& nl, const BatchView& b, const RouteHints& hints, int compute_units,
                                      int resident_blocks, const SolveRequest& closing, bool estimate, bool general, bool careful,
                                      bool samples_wanted) {
  const int derivative = closing.derivative;
  const bool constrained_slots = hints.constrained_slots, moving_starts = hints.moving_starts;
  NonlinearRoute r;
  r.general = general;
  r.careful = careful;
  // the start point is the estimate: computed by the outer-loop kernels themselves (start_time), by a launch of its own in
  // front of the kernels that read their start from a copy
  // (every outer-loop kernel but the one for position-free paths and the careful re-run, which start from a copy of the times)
  r.estimate_in_kernel = estimate && !general && !careful;
  // The split of the four dimensions over lanes is the PLAN's choice (batch size and longest path); this CALL goes back to
  // lane groups where the split kernel would hand its paths to the general step anyway and the groups are 10-25 % faster:
  // 13-15 segments (<= 1536 paths) under an objective order below snap, or when the caller says that vertices hold
  // constrained slots (stop_at waypoints: MRS_TG_FLAG_CONSTRAINED_SLOTS) or mrs_tg_solve_batch has seen a moving start in
  // its host copy of the values.  MRS_TG_REGROUP=0 switches it off.
  const bool regroup = knob::regroup() && nl.regroup_possible && (derivative < 4 || constrained_slots || moving_starts);
  r.dim_split = regroup ? 1 : nl.dim_split;
  const std::vector<NonlinearBin>& plan_bins = regroup ? nl.bins1 : nl.bins;
  r.lean = lean_applies(r.dim_split) && (int)plan_bins.size() <= kMaxBins;
  auto all_fit = [](const std::vector<NonlinearBin>& bins) {
    for (const NonlinearBin& bin : bins)
      if (lean_lds_bytes(bin) > kLdsPerWorkgroup) return false;
    return true;
  };
  // Which lane groups.  The shared half sweeps halve the steps of an evaluation but need S + 4 lanes, the next group width
  // for 13-15 and 29-30 segments: half the paths per wavefront for (S/2 + 1)/S of the steps -- more instructions per path,
  // so a launch of many residency rounds (a saturated device: the kernel is bound by its instruction count) keeps the
  // narrow groups and their one-sided sweeps.  A launch of a few residency rounds lasts about as long as its slowest
  // wavefronts -- ten evaluations of the longest paths -- and there the wide groups win: whole pipeline, wide vs narrow,
  // 8192 ragged 0.57 vs 0.65 ms, 8192 x 14 0.395 vs 0.425, 16384 x 14 0.644 vs 0.674, 32768 x 30 3.33 vs 3.51,
  // 32768 ragged 1.87 vs 1.89; past that narrow: 65536 x 14 2.03 vs 1.97 ms (profiles/round5_wide_groups_ab.txt).
  // (MRS_TG_LEAN_WIDE=0 / 1 forces.)
  // (per device: a process may drive devices of different sizes or partitions, and the first call's figure is not theirs)
  const int resident_waves = compute_units * 4 * MRS_TG_LEAN_WAVES;
  const int lean_shared = knob::lean_shared();
  const int wide_forced = knob::lean_wide_forced();
  const bool lean_masked = derivative < 4;  // rest-to-rest paths end on vertices with free slots
  const bool wide = !nl.wide_bins.empty() && (int)nl.wide_bins.size() <= kMaxBins && !lean_masked && lean_shared != 0 &&
                    (wide_forced >= 0 ? wide_forced == 1 : nl.wide_blocks <= 8 * resident_waves) && all_fit(nl.wide_bins);
  // objective orders below snap: the shared half sweeps with free end slots, every path in a group of S + 4 lanes at least
  // (MRS_TG_LEAN_SHARED=0: the one-sided masked sweeps of optimize_lean_masked_kernel, as until round 5)
  // (a min-snap launch whose caller says that interior vertices may hold constrained slots -- stop_at waypoints -- as well:
  // MRS_TG_FLAG_CONSTRAINED_SLOTS)
  const bool ends_shared = (lean_masked || constrained_slots) && lean_shared != 0 && !nl.ends_bins.empty() &&
                           (int)nl.ends_bins.size() <= kMaxBins && all_fit(nl.ends_bins);
  // min-snap launches of a few residency rounds: EVERY path of two or more segments in a group of S + 4 lanes (the bins of the
  // free-end kernel), so that the kernel with only the shared half sweeps runs -- the one that takes moving starts; 5-7
  // segments then pay 3-4 % for their wider groups when they start at rest (MRS_TG_LEAN_WIDE_ALL=0: only 13-15 and 29-30
  // segments move up and a ragged batch runs the mixed kernel, whose one-sided sweeps leave moving starts to the sweeping kernel)
  const bool wide_shared_all = wide && knob::lean_wide_all() && !nl.ends_bins.empty() && (int)nl.ends_bins.size() <= kMaxBins;
  const std::vector<NonlinearBin>& lean_bins = (ends_shared || wide_shared_all) ? nl.ends_bins : wide ? nl.wide_bins : plan_bins;
  r.lean = r.lean && all_fit(lean_bins);
  if (r.lean) {
    OuterLaunch& L = r.lean_launch;
    L.lds_bytes = fill_bin_table(L.bins, lean_bins, lean_lds_bytes, &L.blocks);
    // A uniform batch of more wavefronts than the device holds at once (two per SIMD): launch what is resident and let a
    // lane group whose path has stopped claim the next one (optimize_body, `queued`), instead of eight rounds of wavefronts
    // that each last as long as the slowest of their four paths.  65536 x 10: 780 -> us.
    if (L.bins.n == 1 && resident_blocks > 0 && L.blocks > resident_blocks) {
      L.blocks = resident_blocks;
      r.queued = true;
    }
    // shared half sweeps (evaluate_lean_shared) where every path of every bin has its S + 4 lanes
    // (with a bin of paths shorter than four segments beside them the kernel that has both evaluations compiled in runs, the
    // short paths in wavefronts of their own next to the others: handing them to the compact kernel BEHIND the launch cost
    // 66 us on 8192 ragged paths, profiles/round5_wide_groups_ab.txt)
    bool lean_shared_only = lean_shared != 0 && !lean_masked;
    bool long_paths = false;  // a bin whose paths have more half sweeps than a wavefront has lanes: the two-pass instantiations
    for (const NonlinearBin& bin : lean_bins) {  // (a bin of one-segment paths: the kernel leaves them to the sweeping kernel behind it)
      if (bin.max_S >= 2 && (bin.min_S < 2 || (bin.max_S + 4 > bin.group && !(bin.group == 64 && bin.max_S <= kLeanTwoPassMaxS))))
        lean_shared_only = false;
      if (bin.max_S + 4 > bin.group && bin.group == 64) long_paths = true;
    }
    const bool ends_long = long_paths && (ends_shared || lean_shared_only);
    r.lean_kernel = ends_long          ? LeanKernel::kLeanSharedEndsLong
                    : ends_shared      ? LeanKernel::kLeanSharedEnds
                    : lean_masked      ? LeanKernel::kLeanMasked
                    : lean_shared_only ? LeanKernel::kLeanShared
                                       : LeanKernel::kLean;
  }
  // one wavefront per path, both directions of the two-sided evaluation in it (mrs_tg_wave.hip)
  if (r.lean || !wave_kernel_applies(b, r.dim_split)) {
    OuterLaunch& L = r.sweep_launch;
    const bool split = r.dim_split == 4;
    // objective order below snap: the end vertices of rest-to-rest paths keep free slots, so the large-batch kernel is
    // launched with the masked step compiled in (the min-snap instantiation stays free of it)
    r.sweep_kernel = split ? SweepKernel::kSplit : derivative < 4 ? SweepKernel::kCompactMasked : SweepKernel::kCompact;
    r.sweep_fits = (int)plan_bins.size() <= kMaxBins;
    if (r.sweep_fits) {
      L.lds_bytes = fill_bin_table(L.bins, plan_bins, [split](const NonlinearBin& bin) { return sweep_lds_bytes(bin, split); }, &L.blocks);
      bool all_single = true;
      for (const NonlinearBin& bin : plan_bins)
        if (bin.group != 64) all_single = false;
      // one path per block and one dimension per lane: a partner wavefront runs the other half of every sweep
      L.threads = (split && all_single) ? 128u : 64u;
      if (L.threads == 128u) L.lds_bytes += (64 * kPairState + 2) * sizeof(double);  // hand-over area + flags
      r.sweep_fits = L.lds_bytes <= kLdsPerWorkgroup;
    }
  }
  r.certified_maxima = knob::maxima_bounds();  // MRS_TG_MAXIMA_BOUNDS=0: every entry searched
  // 2-4 in one launch for the small batches whose wavefronts hold one path (solve_rows_pipeline_kernel, mrs_tg_rows.hip); else
  // 3b + 4 in one launch where the quad kernel (saturated device; the caller's sampler follows) or the rows kernel applies:
  // its staging pass scales the times of its own path, the rows kernel's tail samples.  Paths with a position-free vertex:
  // every stage a launch of its own, the final solve without the waypoints
  r.first_solve = route_solve(b, closing);
  SolveRequest final_request = closing;
  final_request.stage = SolveStage::kClosing;
  final_request.maxima_in_launch = final_request.scale_from_maxima = !general;
  final_request.sampling = samples_wanted && !general;
  final_request.waypoints = closing.waypoints && !general;
  r.final_solve = route_solve(b, final_request);
  return r;
}

}  // namespace mrs_tg

// mrs_tg_nonlinear.h -- launch interface of the segment-time outer loop (internal to the library).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mrs_tg_launch.h"
#include "mrs_tg_nonlinear_route.hpp"
#include "mrs_tg_pool.h"

namespace mrs_tg {

struct NonlinearParams {
  int derivative;
  int max_iterations;
  double f_rel, f_abs, x_rel, x_abs;
  long long time_budget_ticks = 0;  // nlopt maxtime in ticks of the device's constant wall clock (s_memrealtime); 0 = none
  const long long* deadline = nullptr;  // filled in by launch_nonlinear: the call's absolute deadline (device word), or none
  // Paths on which the by-product cost lost its digits (guarded_cost) are listed for the careful re-run
  // (optimize_careful_kernel): position q of the path appended to careful_list (capacity careful_cap) through
  // careful_count; a listed path keeps its start times.  nullptr: no list (the fast kernel's result stands).  A caller of
  // launch_nonlinear only sets careful_cap != 0 to ask for the re-run; the launcher fills in the rest.
  const int32_t* only_flagged = nullptr;  // sweeping kernels: run the paths whose entry (by position) is non-zero only
  int32_t* careful_count = nullptr;
  int32_t* careful_list = nullptr;
  int careful_cap = 0;
  int32_t* queue_next = nullptr;  // lean kernel of a uniform batch larger than the device holds at once: next unclaimed position of the bin
  int ends_min_segments = 2;  // optimize_lean_shared_ends_kernel: shorter paths are left to the sweeping kernel behind it
  int lean_shared = 0;  // lean kernels: shared half sweeps (evaluate_lean_shared) 1: in batches where every path has its S + 4 lanes (own kernel), 2: also wave by wave inside the mixed kernel
  double* sum_t0 = nullptr;  // [n_paths] by path: sum of the times the search starts from (the runaway test of the final solve)
  // The search starts from estimateSegmentTimesEuclidean of these waypoints ([n_vertices][4]) under estimate_limits
  // ([n_paths][9]) instead of from the incoming seg_times: optimize_wave_kernel computes the estimate itself, in front of
  // every other outer-loop kernel launch_nonlinear launches estimate_times_kernel.  nullptr: start from seg_times.
  const double* estimate_wp = nullptr;
  const double* estimate_limits = nullptr;
  const double* pos_wp = nullptr;  // MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: where the saturated-device solves read vertex positions
  bool reference_status = false;   // MRS_TG_FLAG_REFERENCE_STATUS: no runaway test, the outer loop's own code is the path's status
};

struct DfoParams {
  int derivative;
  int mode;            // 0 squared time, 1 Richter time, 3 / 4 the same with the free constraints as variables
  int max_iterations;
  double f_rel, f_abs, x_rel, x_abs;
  double time_penalty, soft_weight;
  int use_soft;
  double initial_stepsize_rel;
  long long time_budget_ticks = 0;  // as NonlinearParams
};

// (its device blocks go back to the pool with the plan: mrs_tg_plan_destroy synchronises, then deletes)
struct NonlinearPlan {
  NonlinearHostPlan host;            // the lane-group bins and the dimension split (nonlinear_host_plan, mrs_tg_nonlinear_route.hpp)
  DeviceBlock<double> d_ws;          // factor store of the per-lane linear solve
  DeviceBlock<int32_t> d_opt_status; // stopping reason of the outer loop per path
  DeviceBlock<double> d_maxima;      // [n_segments][9] per-segment maxima
  DeviceBlock<int32_t> d_queue;      // the lean kernel's path queue (one counter)
  DeviceBlock<double> d_sum_t0;      // [n_paths] sum of the times the outer loop started from (runaway test)
  DeviceBlock<int32_t> d_fallback;   // [n_paths] by position: 1 = the prefix / suffix kernel left the path to the sweeping kernel
  DeviceBlock<int32_t> d_careful;    // [0] count, [2] count of the last completed call, [4..] list of guarded paths
  DeviceBlock<double> d_careful_ws;  // factor store of optimize_careful_kernel's lanes
  // paths with a position-free vertex (MRS_TG_FLAG_GENERAL_PATTERNS), allocated on first use
  DeviceBlock<int32_t> d_general;          // [0] count | [4 + p] flag by path | [4 + n_paths + k] list of positions
  DeviceBlock<double> d_general_ws;        // factor store of optimize_general_kernel's lanes
  DeviceBlock<double> d_general_solve_ws;  // factor store of solve_general_kernel (general_workspace_doubles)
  DeviceBlock<double> d_general_t0;        // [n_segments] the times the call started from
  // gradient-free modes (0, 1, 3, 4), allocated on first use
  DeviceBlock<double> d_dfo_vec;       // x | x0 | best | h | lb | ub, each 21 n_segments + 20 n_paths doubles
  DeviceBlock<double> d_dfo_f;         // fbest | f_sweep | J_d scratch, 3 * n_paths doubles
  DeviceBlock<int32_t> d_dfo_state;    // phase, i, sg, neval, improved, ret, done, n_var per path
  DeviceBlock<int32_t> d_dfo_fidx;     // modes 3/4: free-constraint index of every (vertex, derivative), -1 if fixed
  DeviceBlock<double> d_dfo_segcost;   // modes 3/4: J_d share of every (segment, dimension)
  DeviceBlock<int32_t> d_dfo_seg_path; // modes 3/4: path of every segment
  DeviceBlock<long long> d_dfo_deadline; // wall-clock deadline of the running search (0 = none), written by its first kernel
};

// shared by the launchers of mrs_tg_nonlinear.hip and mrs_tg_dfo.hip: the plan's lazily allocated buffers, and the flags / list
// of a call's paths with a position-free vertex (`outer_loop`: also what optimize_general_kernel needs; *cap = paths per launch)
hipError_t nonlinear_ensure_buffers(NonlinearPlan& nl, const BatchView& b);
hipError_t nonlinear_prepare_general(NonlinearPlan& nl, const BatchView& b, const uint8_t* mask, const double* seg_times,
                                     bool outer_loop, int* cap, hipStream_t stream);

// whether optimize_careful_kernel (MRS_TG_FLAG_CAREFUL_COST) is in this build (-DMRS_TG_WITH_CAREFUL=1)
bool careful_rerun_built();

// general: paths with a position-free vertex may occur (MRS_TG_FLAG_GENERAL_PATTERNS); they take the 5 x 5-block route
// (optimize_general_kernel / solve_general_kernel) behind the fast kernels, the others are untouched by it.
// sampling_dt > 0: the caller wants the result sampled; when the final solve runs on the rows kernel the sampling rides
// on that launch (*sampled_out = true) and the caller must not launch the sampler again
// hints: the call's (RouteHints, mrs_tg_transfer.hpp), for the outer loop's route and for every solve either launcher runs
hipError_t launch_nonlinear(NonlinearPlan& nl, const BatchView& b, const RouteHints& hints, const NonlinearParams& prm,
                            const uint8_t* mask, const double* vals, const double* limits, double* seg_times, double* coeffs,
                            int32_t* status, double* cost, hipStream_t stream, double sampling_dt = 0.0,
                            int sample_capacity = 0, int32_t* n_samples = nullptr, double* samples = nullptr,
                            bool* sampled_out = nullptr, bool general = false);
hipError_t launch_dfo(NonlinearPlan& nl, const BatchView& b, const RouteHints& hints, const DfoParams& prm, const uint8_t* mask,
                      const double* vals, const double* limits, double* seg_times, double* coeffs, int32_t* status, double* cost,
                      hipStream_t stream, bool general = false);
hipError_t launch_cost_gradient(NonlinearPlan& nl, const BatchView& b, int d, const uint8_t* mask, const double* vals,
                                const double* seg_times, double* cost, double* grad, hipStream_t stream);
hipError_t launch_segment_maxima(const BatchView& b, const double* coeffs, const double* seg_times, double* maxima,
                                 hipStream_t stream);

}  // namespace mrs_tg

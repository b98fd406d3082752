// mrs_tg_launch.h -- host-visible view of a batch and the kernel launchers (internal to the library).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mrs_tg.h"
#include "mrs_tg_batch.hpp"
#include "mrs_tg_hd.hpp"
#include "mrs_tg_knobs.hpp"
#include "mrs_tg_solve_route.hpp"
#include "mrs_tg_transfer.hpp"

struct mrs_tg_ctx;

namespace mrs_tg {

namespace pathq {
struct ThinOptions;  // mrs_tg_pathedit.hpp
}
namespace fldq {
struct Geometry;  // mrs_tg_field.hpp
}
namespace edtq {
struct Weights;     // mrs_tg_edt.hpp
struct RegionPlan;  // mrs_tg_edt_region.hpp
}

// Per-dispatch timing (mrs_tg_set_profiling): the next launch of the kernel family a ProfileScope names carries these
// events on the launch itself (hipExtLaunchKernelGGL), so their difference is the dispatch's own start-to-end time.
struct KernelTimer {
  hipEvent_t start = nullptr, stop = nullptr;
};
KernelTimer take_kernel_timer();  // the pending pair (null events when nothing is pending); consumed by the call
void set_kernel_timer(hipEvent_t start, hipEvent_t stop);  // arms the next timed launch of this thread
// (RouteHints, what a solve tells its launchers beside the batch and the options: mrs_tg_transfer.hpp.  Every launcher that
// reads a hint, or calls one that does, takes them as an argument without a default.)
// compute units of the calling thread's current device, looked up once per device ordinal (a process may drive devices of
// different sizes or partitions); 256 while the runtime cannot say
int device_compute_units();
// Kernel trace (mrs_tg_kernel_trace): every launch of the library notes its kernel's name in a small per-thread ring, so
// that a test or the benchmark can SAY which kernels a call ran instead of inferring it from batch sizes (one pointer store)
void note_kernel(const char* name);
void kernel_trace_reset();
int kernel_trace(const char** names_out, int capacity);  // oldest first; at most the newest 32 since the reset
// Dry run (mrs_tg_plan_explain): the calling thread's launchers run their routing -- every size rule, environment knob and
// hint exactly as in a real call -- and NOTE the kernels they would launch, but enqueue nothing
bool dry_run();
void set_dry_run(bool on);
// One kernel of a launcher's choice: the host function with the name that note_kernel records.  The instantiations a launcher
// chooses between share one signature, so the choice is an ordinary ?: over these values, made once and handed to both
// hipFuncSetAttribute (set_max_dynamic_lds) and the launch.  MRS_TG_KERNEL(solve_quad_kernel<false, true>) notes exactly that
// text, and MRS_TG_KERNEL((solve_linear_kernel<1, true>)) its parentheses too: the names are interface (mrs_tg_kernel_trace,
// mrs_tg_plan_explain) and stay as they always were; a name no expression spells goes to kernel_as directly.
template <class... Args>
struct Kernel {
  void (*fn)(Args...);
  const char* name;
};
template <class... Args>
constexpr Kernel<Args...> kernel_as(void (*fn)(Args...), const char* name) { return {fn, name}; }
#define MRS_TG_KERNEL(...) ::mrs_tg::kernel_as(__VA_ARGS__, #__VA_ARGS__)
// (the launch macros take a Kernel or a kernel written in place, which is noted as written)
template <class... Args>
constexpr auto kernel_fn(const Kernel<Args...>& k) { return k.fn; }
template <class... Args>
constexpr auto kernel_fn(void (*fn)(Args...)) { return fn; }
template <class... Args>
constexpr const char* kernel_name(const Kernel<Args...>& k, const char*) { return k.name; }
template <class... Args>
constexpr const char* kernel_name(void (*)(Args...), const char* written) { return written; }
template <class... Args>
inline hipError_t set_max_dynamic_lds(const Kernel<Args...>& k, size_t bytes) {
  return hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// The dynamic LDS of a launch (kLdsPerWorkgroup, kLdsDefaultLimit: mrs_tg_solve_route.hpp): a workgroup cannot have more than a
// compute unit's 160 KB (hipErrorInvalidValue, which the ABI words for its caller), and more than the 64 KB a launch may ask for
// by default needs the kernel's limit raised first (a driver call, so only then).  A launcher that returns early for an empty
// batch refuses an oversize need before it does.
template <class... Args>
inline hipError_t prepare_dynamic_lds(const Kernel<Args...>& k, size_t bytes) {
  if (bytes > kLdsPerWorkgroup) return hipErrorInvalidValue;
  return bytes > kLdsDefaultLimit ? set_max_dynamic_lds(k, bytes) : hipSuccess;
}
// an empty batch launches nothing, but still refuses an oversize LDS need (what a launcher with dynamic LDS returns for it)
inline hipError_t empty_batch_lds(size_t bytes) { return bytes > kLdsPerWorkgroup ? hipErrorInvalidValue : hipSuccess; }
// workgroups of `b` items that cover `a`
inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
// launch with the pending timer, if any
#define MRS_TG_LAUNCH_TIMED(kernel, grid, block, lds, stream, ...)                                           \
  do {                                                                                                       \
    const ::mrs_tg::KernelTimer kt__ = ::mrs_tg::take_kernel_timer();                                        \
    ::mrs_tg::note_kernel(::mrs_tg::kernel_name(kernel, #kernel));                                           \
    if (!::mrs_tg::dry_run())                                                                                \
      hipExtLaunchKernelGGL(::mrs_tg::kernel_fn(kernel), grid, block, lds, stream, kt__.start, kt__.stop, 0, __VA_ARGS__); \
  } while (0)
// plain launches, and launches that carry the events of a multi-kernel timing themselves
#define MRS_TG_LAUNCH(kernel, ...)                                                    \
  do {                                                                                \
    ::mrs_tg::note_kernel(::mrs_tg::kernel_name(kernel, #kernel));                    \
    if (!::mrs_tg::dry_run()) {                                                       \
      const auto fn__ = ::mrs_tg::kernel_fn(kernel);                                  \
      hipLaunchKernelGGL(fn__, __VA_ARGS__);                                          \
    }                                                                                 \
  } while (0)
#define MRS_TG_LAUNCH_EXT(kernel, ...)                                                \
  do {                                                                                \
    ::mrs_tg::note_kernel(::mrs_tg::kernel_name(kernel, #kernel));                    \
    if (!::mrs_tg::dry_run()) hipExtLaunchKernelGGL(::mrs_tg::kernel_fn(kernel), __VA_ARGS__);   \
  } while (0)

// records `message` as the context's (and the global) last error and returns `code`
int report_error(mrs_tg_ctx* ctx, int code, const char* fmt, ...);
// pinned host scratch owned by the context (grown on demand, kept across calls, freed with the context); null when the
// runtime refuses the allocation
void* ctx_host_scratch(mrs_tg_ctx* ctx, size_t bytes);
// mrs_tg_solve_batch for a caller that reads only times, statuses and samples: the coefficients are not downloaded
int solve_batch_samples_only(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* seg_offsets, const double* waypoints,
                             const uint8_t* fixed_mask, const double* fixed_values, const double* limits,
                             const mrs_tg_options* opt, double* seg_times_inout, int32_t* status_out, int32_t* n_samples_out,
                             double* samples_out);

// (BatchView, the device-resident structure of a batch: mrs_tg_batch.hpp)
hipError_t launch_assemble(const BatchView& b, int d, const double* seg_times, double* H, double* Ainv,
                           hipStream_t stream);
// (CopyList, up to kCopyMax flat copies in ONE launch: mrs_tg_transfer.hpp)
hipError_t launch_copy_many(const CopyList& cl, hipStream_t stream);
// samples [n_paths][capacity][4]: only the min(n_samples[p], capacity) rows a path has produced are copied (a sample buffer
// is sized for the longest trajectory the caller would accept; a typical one uses a fraction of it)
hipError_t launch_copy_samples(const double* src, double* dst, const int32_t* n_samples, int n_paths, int capacity,
                               hipStream_t stream);

// (timed: the launch carries the pending ProfileScope's events -- mrs_tg_plan_estimate_times, where the estimate is the call's
// own kernel; inside a solve it is a prelude and leaves the timer to the solve)
hipError_t launch_estimate_times(const BatchView& b, const double* wp, const double* limits, double* seg_times,
                                 hipStream_t stream, bool timed = false);
// (one wavefront per path: sample_kernel)
hipError_t launch_sample(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                         int32_t* n_samples, double* samples, hipStream_t stream);
// the same walk, every sample with its derivative orders 0..4: states [n_paths][capacity][kSampleStateOrders][4]
constexpr int kSampleStateOrders = kMaxOrders;
// the rows of the state kernels carry the position alone or every order: any other n_orders is refused (hipErrorInvalidValue)
constexpr bool valid_state_orders(int n_orders) { return n_orders == 1 || n_orders == kSampleStateOrders; }
hipError_t launch_sample_states(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                                int32_t* n_samples, double* states, hipStream_t stream);
// ---- the policy layer's per-round device work (mrs_tg_policy_dev.hip) ----
// constraint mask [n_vertices][5] and values [n_vertices][5][4] from the unwrapped waypoints [n_vertices][4], vinfo[v] = position of
// the vertex's path in the round's batch << 4 | flags, and the initial states [n_paths][12] (velocity, acceleration, jerk)
hipError_t launch_policy_expand(int n_vertices, int d, const double* wp, const int32_t* vinfo, const double* init, uint8_t* mask,
                                double* vals, hipStream_t stream);
struct PolicyValidateArgs {
  int n_paths;
  const int32_t* seg_offsets;   // [n_paths + 1] (device)
  const double* wp;             // [sum V][4]
  const double* samples;        // [n_paths][capacity][4]
  const int32_t* n_samples;     // [n_paths] as the solve reported them
  const int32_t* status;        // [n_paths]
  const double* baca_total;     // [n_paths] initial_total_time_baca
  double dt, max_len_factor, min_len_factor, max_deviation;
  int capacity, first_segment, check_enabled, last_round;
  // results (any address the device can write: pinned host memory)
  int32_t* ok_out;
  int32_t* ns_out;
  int32_t* status_out;
  double* max_dev_out;
  uint8_t* is_safe_out;
  uint8_t* safe_out;            // [sum S]
  int32_t* ns_copy;             // [n_paths] (device) rows of the finished paths' samples that travel
};
hipError_t launch_policy_validate(const PolicyValidateArgs& args, hipStream_t stream);

size_t linear_workspace_doubles(const BatchView& b);
// MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS, checked: the number of vertices whose position is unconstrained or whose constrained
// position differs (bitwise) from its waypoint.  Blocks until the count is on the host.
hipError_t count_position_mismatches(const BatchView& b, const double* wp, const uint8_t* mask, const double* vals,
                                     hipStream_t stream, long long* count_out);
// any fixed / free pattern, position-free vertices included (mrs_tg_general.hip): solves the paths flagged in `only` (by
// path, non-zero) or, without it, the paths whose status is -2; status out = 1 or opt_status' stopping reason
size_t general_workspace_doubles(const BatchView& b);
hipError_t launch_solve_general(const BatchView& b, int d, const uint8_t* mask, const double* vals, const double* seg_times,
                                double* ws, double* coeffs, int32_t* status, double* cost, hipStream_t stream,
                                const int32_t* only = nullptr, const int32_t* opt_status = nullptr);
// MRS_TG_FLAG_REFINE (mrs_tg_refine.hip): every path with status > 0 refined at its segment times -- coeffs and cost (may be
// NULL) rewritten, seg_times and status read only; per-lane factors and iterates in `ws` (refine_workspace_doubles)
size_t refine_workspace_doubles(const BatchView& b);
hipError_t launch_refine(const BatchView& b, int d, const uint8_t* mask, const double* vals, const double* seg_times, double* ws,
                         double* coeffs, const int32_t* status, double* cost, hipStream_t stream);
// mrs_tg_plan_solve_vjp (mrs_tg_vjp.hip): the backward pass of the fixed-times solve -- dL/dfixed_values and dL/dseg_times
// (either may be NULL) from dL/dcoeffs and dL/dcost (either may be NULL = zero); reads only; per-lane factors in `ws`
// (vjp_workspace_doubles); timed as the kernel family of the pending ProfileScope
size_t vjp_workspace_doubles(const BatchView& b);
hipError_t launch_vjp(const BatchView& b, int d, const uint8_t* mask, const double* vals, const double* seg_times,
                      const double* coeffs, const int32_t* status, const double* grad_coeffs, const double* grad_cost, double* ws,
                      double* grad_vals, double* grad_times, hipStream_t stream);
// mrs_tg_plan_segment_maxima_vjp (mrs_tg_maxima_vjp.hip): the backward pass of the segment maxima -- dL/dcoeffs, dL/dseg_times
// and the maximisers t* (each may be NULL) from dL/dmaxima; reads only, no workspace; timed as the kernel family of the
// pending ProfileScope
hipError_t launch_segment_maxima_vjp(int n_segments, const double* coeffs, const double* seg_times, const double* grad_maxima,
                                     double* grad_coeffs, double* grad_times, double* argmax, hipStream_t stream);
// mrs_tg_plan_sample_states_vjp (mrs_tg_sample_vjp.hip): the backward pass of the sampler -- dL/dcoeffs and dL/dseg_times from
// dL/dsamples (grad_states [n_paths][capacity][n_orders][4], n_orders 1 or kSampleStateOrders), the (segment, time) of every
// sample and the counts (each output may be NULL); status NULL or per path (<= 0: zero rows); reads only, no workspace; timed as
// the kernel family of the pending ProfileScope
hipError_t launch_sample_vjp(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                             int n_orders, const double* grad_states, const int32_t* status, double* grad_coeffs,
                             double* grad_times, int32_t* sample_segment, double* sample_time, int32_t* n_samples,
                             hipStream_t stream);
// mrs_tg_plan_evaluate / mrs_tg_plan_evaluate_vjp (mrs_tg_evaluate.hip): the state of every path at caller-given times
// (query_times [n_paths][n_queries] in the caller's path order, states [n_paths][n_queries][n_orders][4], n_orders 1 or
// kSampleStateOrders; query_segment / query_tau [n_paths][n_queries] may be NULL) and its backward pass -- dL/dcoeffs,
// dL/dseg_times and dL/dquery_times (each may be NULL) from dL/dstates; status NULL or per path (<= 0: zero rows); reads only,
// no workspace; each timed as the kernel family of the pending ProfileScope
hipError_t launch_evaluate(const BatchView& b, const double* coeffs, const double* seg_times, const double* query_times,
                           int n_queries, int n_orders, double* states, int32_t* query_segment, double* query_tau,
                           hipStream_t stream);
hipError_t launch_evaluate_vjp(const BatchView& b, const double* coeffs, const double* seg_times, const double* query_times,
                               int n_queries, int n_orders, const double* grad_states, const int32_t* status,
                               double* grad_coeffs, double* grad_times, double* grad_query, hipStream_t stream);
// mrs_tg_plan_path_deviation / mrs_tg_plan_path_deviation_vjp (mrs_tg_deviation.hip): the deviation of the samples
// [n_paths][capacity][4] from the waypoint polyline [sum V][4] by validateTrajectorySpatial's scan (every output may be NULL)
// and its backward pass -- dL/dsamples and dL/dwaypoints (each may be NULL) from dL/ddeviation; status NULL or per path
// (<= 0: zero rows); reads only, no workspace; each timed as the kernel family of the pending ProfileScope
hipError_t launch_path_deviation(const BatchView& b, const double* samples, const int32_t* n_samples, const double* waypoints,
                                 int capacity, int first_segment, const int32_t* status, double* deviation, int32_t* cursor,
                                 double* max_deviation, int32_t* argmax, double* segment_max, hipStream_t stream);
hipError_t launch_path_deviation_vjp(const BatchView& b, const double* samples, const int32_t* n_samples,
                                     const double* waypoints, int capacity, const int32_t* status, const double* grad_deviation,
                                     double* grad_samples, double* grad_waypoints, hipStream_t stream);
// mrs_tg_plan_waypoint_passage / mrs_tg_plan_waypoint_passage_vjp (mrs_tg_passage.hip): where the samples [n_paths][capacity][4]
// pass the waypoints by getWaypointInTrajectoryIdxs' scan -- index, count, miss distance and foot point per waypoint (every
// output may be NULL) -- and its backward pass: dL/dsamples and dL/dwaypoints (each may be NULL) from dL/dmiss and dL/dfraction
// (each may be NULL = zero).  wp_offsets [n_paths + 1] (device) with waypoints [sum W][4], or NULL: the plan's own vertices.
// status NULL or per path (<= 0: nothing reached, zero rows); reads only, no workspace, no LDS; each timed as the kernel
// family of the pending ProfileScope
hipError_t launch_waypoint_passage(const BatchView& b, const double* samples, const int32_t* n_samples, int capacity,
                                   const int32_t* wp_offsets, const double* waypoints, const int32_t* status, int32_t* index,
                                   int32_t* count, double* miss, double* fraction, hipStream_t stream);
hipError_t launch_waypoint_passage_vjp(const BatchView& b, const double* samples, const int32_t* n_samples, int capacity,
                                       const int32_t* wp_offsets, const double* waypoints, const int32_t* status,
                                       const double* grad_miss, const double* grad_fraction, double* grad_samples,
                                       double* grad_waypoints, hipStream_t stream);
// mrs_tg_plan_estimate_times_vjp (mrs_tg_estimate_vjp.hip): the backward pass of the Euclidean segment-time estimate --
// dL/dwaypoints [sum V][4], dL/dlimits [n_paths][9] and the term of every segment [sum S] (each may be NULL) from dL/dseg_times
// (may be NULL when only the terms are wanted); reads only, no workspace; timed as the kernel family of the pending ProfileScope
hipError_t launch_estimate_times_vjp(const BatchView& b, const double* wp, const double* limits, const double* grad_times,
                                     double* grad_wp, double* grad_limits, int32_t* term, hipStream_t stream);
// mrs_tg_plan_estimate_times_baca / mrs_tg_plan_estimate_times_baca_vjp / mrs_tg_plan_length_gate (mrs_tg_baca.hip): the Baca
// segment-time estimate [sum S] of waypoints [sum V][4] under limits [n_paths][9]; its backward pass -- dL/dwaypoints, dL/dlimits
// and the flags of every segment [sum S] (each may be NULL) from dL/dseg_times (may be NULL when only the flags are wanted); and
// the length gate: per path the total of seg_times and the verdict on n_samples * dt (either may be NULL; status may be NULL).
// Reads only, no workspace, no LDS; each timed as the kernel family of the pending ProfileScope
hipError_t launch_baca_times(const BatchView& b, const double* wp, const double* limits, double* seg_times, hipStream_t stream);
hipError_t launch_baca_times_vjp(const BatchView& b, const double* wp, const double* limits, const double* grad_times,
                                 double* grad_wp, double* grad_limits, int32_t* flags, hipStream_t stream);
hipError_t launch_length_gate(const BatchView& b, const double* seg_times, const int32_t* n_samples, double dt, double max_factor,
                              double min_factor, const int32_t* status, double* total, int32_t* verdict, hipStream_t stream);
// mrs_tg_plan_unwrap_headings / mrs_tg_plan_fallback_sample / mrs_tg_plan_fallback_sample_vjp (mrs_tg_fallback.hip): the headings
// of waypoints [sum V][4] unwrapped along every path (out may be wp); the fallback sampler's rows [n_paths][capacity][4] of the
// waypoint polyline on seg_times [sum S] with `insert` repeated rows at a stop_at waypoint (stop_at [sum V] and seg_first_row
// [sum S] may be NULL); and its backward pass, dL/dwaypoints [sum V][4] from dL/dsamples.  Reads only, no workspace, LDS sized by the plan's longest path;
// each timed as the kernel family of the pending ProfileScope
hipError_t launch_unwrap_headings(const BatchView& b, const double* wp, double* out, hipStream_t stream);
hipError_t launch_fallback_sample(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const double* seg_times,
                                  double dt, int insert, int capacity, int32_t* n_samples, double* samples,
                                  int32_t* seg_first_row, hipStream_t stream);
hipError_t launch_fallback_sample_vjp(const BatchView& b, const uint8_t* stop_at, const double* seg_times, double dt, int insert,
                                      int capacity, const double* grad_samples, double* grad_waypoints, hipStream_t stream);
// mrs_tg_plan_preprocess_path / mrs_tg_plan_insert_midpoints / mrs_tg_plan_path_edit_vjp (mrs_tg_pathedit.hip): the two steps that
// change the number of vertices of a path -- preprocessPath's thinning of waypoints [sum V][4] and the mid-points of the segments
// whose segment_max [sum S] exceeds max_deviation (active [n_paths] may be NULL: every path) -- each as a PACKED batch: offsets
// [n_paths + 1] (written: the edited paths' first vertices and their total), waypoints_out, stop_out, source_out, inserted_out
// (rows below offsets[n_paths] written once; the last three may be NULL); ws: one int32 per vertex of the plan.  Three launches
// each (decide and count per path, one workgroup for the offsets, one lane per output vertex), timed from the first to the last
// as the kernel family of the pending ProfileScope.  Their backward pass: dL/dwaypoints [sum V][4] from dL/dedited rows.
constexpr int kPathEditScanChunk = 1024;  // paths the offsets' one workgroup takes at a time
hipError_t launch_preprocess_path(const BatchView& b, const double* waypoints, const uint8_t* stop_at,
                                  const pathq::ThinOptions& o, int32_t* ws, int32_t* offsets, double* waypoints_out,
                                  uint8_t* stop_out, int32_t* source_out, hipStream_t stream);
hipError_t launch_insert_midpoints(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const double* segment_max,
                                   double max_deviation, int first_segment, const uint8_t* active, int32_t* ws, int32_t* offsets,
                                   double* waypoints_out, uint8_t* stop_out, int32_t* source_out, uint8_t* inserted_out,
                                   hipStream_t stream);
hipError_t launch_path_edit_vjp(const BatchView& b, const int32_t* offsets, const int32_t* source, const uint8_t* inserted,
                                const double* grad_edited, double* grad_waypoints, hipStream_t stream);
// the one workgroup that turns the counts at offsets[1 ..] into offsets (vertex_offsets_kernel), for an edit that counts by itself;
// start / stop: the events of the caller's multi-launch timing that fall on this launch (may be null)
hipError_t launch_vertex_offsets(int n_paths, int32_t* offsets, hipEvent_t start, hipEvent_t stop, hipStream_t stream);
// mrs_tg_plan_initial_condition, mrs_tg_plan_prepend_initial_condition, mrs_tg_plan_splice_prediction and their backward passes
// (mrs_tg_initial.hip, mrs_tg_initial.hpp): the state a trajectory starts from, per path, from the tracker command, the UAV state
// or row k of the prediction pred[0 .. 3] = position, velocity, acceleration, jerk [n_paths][pred_capacity][4]; the edit that
// drops the first requested vertex and puts row 0 of that state in front, packed as the path edits pack (three launches, timed
// from the first to the last); the k prediction rows in front of the samples of a path from the future, in place or out of
// place.  The requested vertices are addressed by vertex_offsets [n_paths + 1] (n_vertices = vertex_offsets[n_paths]); a path
// may have none.  Backward: copies and zeros.  Each timed as the kernel family of the pending ProfileScope.
hipError_t launch_initial_condition(int n_paths, const int32_t* flags, const double* tracker, const double* tracker_age,
                                    const double* uav_pose, double takeoff_height, const double* path_time_offset,
                                    const int32_t* vertex_offsets, const double* const pred[4], const int32_t* n_pred,
                                    int pred_capacity, int32_t* decision_out, int32_t* sample_offset_out, double* initial_out,
                                    hipStream_t stream);
hipError_t launch_initial_condition_vjp(int n_paths, const int32_t* decision, const int32_t* sample_offset,
                                        const double* grad_initial, int pred_capacity, double* grad_tracker, double* grad_uav,
                                        double* const grad_pred[4], hipStream_t stream);
hipError_t launch_prepend_initial_condition(int n_paths, int n_vertices, const int32_t* vertex_offsets, const double* waypoints,
                                            const uint8_t* stop_at, const int32_t* decision, const double* initial,
                                            int32_t* offsets, double* waypoints_out, uint8_t* stop_out, int32_t* source_out,
                                            hipStream_t stream);
hipError_t launch_prepend_initial_condition_vjp(int n_paths, int n_vertices, const int32_t* vertex_offsets, const int32_t* decision,
                                                const int32_t* offsets, int n_edited, const double* grad_edited,
                                                double* grad_waypoints, double* grad_initial_row, hipStream_t stream);
hipError_t launch_splice_prediction(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                    const int32_t* status, const int32_t* decision, const int32_t* sample_offset,
                                    const double* prediction_age, const double* pred_position, const int32_t* n_pred,
                                    int pred_capacity, double* samples_out, int32_t* n_samples_out, int32_t* status_out,
                                    hipStream_t stream);
hipError_t launch_splice_prediction_vjp(int n_paths, const int32_t* n_samples, int capacity, const int32_t* status,
                                        const int32_t* decision, const int32_t* sample_offset, const double* prediction_age,
                                        const int32_t* n_pred, int pred_capacity, const double* grad_out, double* grad_samples,
                                        double* grad_pred_position, hipStream_t stream);
// mrs_tg_plan_travel_heading / mrs_tg_plan_travel_heading_vjp (mrs_tg_heading.hip): the heading of the rows 0 .. n-2 of samples
// [n_paths][capacity][4] set to the direction of the step to the next row, a row that moves less than min_step keeping the
// heading in front of it (samples_out may be samples; source_out [n_paths][capacity] may be NULL); and its backward pass,
// dL/dsamples from the upstream on the output rows, the sources held fixed.  One wavefront per path; reads only, no LDS, no
// workspace; each timed as the kernel family of the pending ProfileScope
hipError_t launch_travel_heading(int n_paths, const double* samples, const int32_t* n_samples, int capacity, const int32_t* status,
                                 double min_step, double* samples_out, int32_t* source_out, hipStream_t stream);
hipError_t launch_travel_heading_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                     const int32_t* status, double min_step, const double* grad_out, double* grad_samples,
                                     hipStream_t stream);
// mrs_tg_plan_request_vertices / mrs_tg_plan_request_limits and their backward passes (mrs_tg_request.hip, mrs_tg_request.hpp): the
// vertices findTrajectory builds from the raw waypoints [sum V][4] -- headings unwrapped along every path from the state's
// heading (state [n_paths][4][4], has_state [n_paths] or null: none), mask [sum V][5], values [sum V][5][4]; every output may be
// null, waypoints_out may be waypoints -- and the limits [n_paths][9] with their branch word from constraints [n_paths][12], the
// override [n_paths][6] (read where flags says so) and the fallback's factors.  Backward: copies, one addition per waypoint entry,
// one multiplication per scaled limit; every element of every output written once.  One wavefront per path (vertices), one lane
// per vertex (their backward pass), one lane per path (limits); no LDS, no workspace; each timed as the kernel family of the
// pending ProfileScope
hipError_t launch_request_vertices(const BatchView& b, const double* waypoints, const uint8_t* stop_at, const uint8_t* has_state,
                                   const double* state, int d, double* waypoints_out, uint8_t* mask, double* vals,
                                   hipStream_t stream);
hipError_t launch_request_vertices_vjp(const BatchView& b, const uint8_t* has_state, const double* grad_wp, const double* grad_vals,
                                       double* grad_raw, double* grad_state, hipStream_t stream);
hipError_t launch_request_limits(int n_paths, const double* constraints, const double* override_, const int32_t* flags,
                                 const uint8_t* has_state, const double* state, int fallback, double speed_factor,
                                 double accel_factor, double* limits, int32_t* branch, hipStream_t stream);
hipError_t launch_request_limits_vjp(int n_paths, const int32_t* branch, int fallback, double speed_factor, double accel_factor,
                                     const double* grad_limits, double* grad_constraints, double* grad_override,
                                     hipStream_t stream);
// mrs_tg_plan_mutual_clearance / mrs_tg_plan_mutual_clearance_vjp (mrs_tg_clearance.hip, mrs_tg_clearance.hpp): per row of samples
// [n_paths][capacity][4] the distance to the nearest other path of the row's group at the same common step (group_offsets
// [n_groups + 1], first_step [n_paths] or null: all 0; z_scale weighs the vertical separation) and that path's index, per path
// the minimum over its rows and where it is (every output may be null); and its backward pass, dL/dsamples from dL/dclearance
// with the partners held fixed, a gather.  status null or per path (<= 0: no rows, nobody's neighbour).  One workgroup per path;
// reads only, no workspace, no dynamic LDS; each timed as the kernel family of the pending ProfileScope
hipError_t launch_mutual_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                   const int32_t* group_offsets, int n_groups, const int32_t* first_step, const int32_t* status,
                                   double z_scale, double* clearance, int32_t* partner, double* min_clearance, int32_t* argmin,
                                   hipStream_t stream);
hipError_t launch_mutual_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                       const int32_t* group_offsets, int n_groups, const int32_t* first_step,
                                       const int32_t* status, double z_scale, const int32_t* partner, const double* grad_clearance,
                                       double* grad_samples, hipStream_t stream);
// mrs_tg_plan_obstacle_clearance / mrs_tg_plan_obstacle_clearance_vjp (mrs_tg_obstacle.hip, mrs_tg_obstacle.hpp): per row of samples
// [n_paths][capacity][4] the signed distance to the nearest obstacle of the path's set -- obstacles [n_obstacles][4] = (x, y, z,
// radius), partitioned into sets by set_offsets [n_sets + 1], path_set [n_paths] or null: every path sees set 0; z_scale weighs
// the vertical separation -- and that obstacle's index in the whole array, per path the minimum over its rows and where it is
// (every output may be null); and its backward pass, dL/dsamples from dL/dclearance with the nearest obstacles held fixed.
// status null or per path (<= 0: no rows).  One workgroup per path; reads only, no workspace, no dynamic LDS; each timed as the
// kernel family of the pending ProfileScope
hipError_t launch_obstacle_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                     const double* obstacles, int n_obstacles, const int32_t* set_offsets, int n_sets,
                                     const int32_t* path_set, const int32_t* status, double z_scale, double* clearance,
                                     int32_t* nearest, double* min_clearance, int32_t* argmin, hipStream_t stream);
hipError_t launch_obstacle_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                         const double* obstacles, int n_obstacles, const int32_t* set_offsets, int n_sets,
                                         const int32_t* path_set, const int32_t* status, double z_scale, const int32_t* nearest,
                                         const double* grad_clearance, double* grad_samples, hipStream_t stream);
// mrs_tg_plan_field_clearance / mrs_tg_plan_field_clearance_vjp (mrs_tg_field.hip, mrs_tg_field.hpp): per row of samples
// [n_paths][capacity][4] the trilinear interpolant of the voxel grid of signed distances the path sees -- fields
// [n_fields][nz][ny][nx] of one geometry, path_field [n_paths] or null: every path sees grid 0; outside_value for a live row
// outside the grid -- the low corner's index in the whole array, the field's gradient [n_paths][capacity][4], per path the
// minimum over its rows and where it is (every output may be null); and its backward pass, dL/dsamples from dL/dclearance with
// the cells held fixed.  status null or per path (<= 0: no rows).  One workgroup per path; reads only, no workspace, no dynamic
// LDS; each timed as the kernel family of the pending ProfileScope
hipError_t launch_field_clearance(int n_paths, const double* samples, const int32_t* n_samples, int capacity, const double* fields,
                                  const fldq::Geometry& geometry, const int32_t* path_field, const int32_t* status,
                                  double outside_value, double* clearance, int32_t* cell, double* gradient, double* min_clearance,
                                  int32_t* argmin, hipStream_t stream);
hipError_t launch_field_clearance_vjp(int n_paths, const double* samples, const int32_t* n_samples, int capacity,
                                      const double* fields, const fldq::Geometry& geometry, const int32_t* path_field,
                                      const int32_t* status, const int32_t* cell, const double* grad_clearance,
                                      double* grad_samples, hipStream_t stream);
// mrs_tg_field_from_occupancy (mrs_tg_edt.hip, mrs_tg_edt.hpp): occupancy [n_fields][nz][ny][nx] bytes (non-zero: occupied) ->
// fields [n_fields][nz][ny][nx] doubles, the exact Euclidean distance to the nearest occupied node with the weights W, capped at
// max_distance (limit: edtq::saturation(max_distance)); is_signed: minus the distance to the nearest free node at the occupied
// ones.  dims = nx, ny, nz, each in [2, edtq::kMaxDim].  Three launches (edt_x_kernel, edt_y_kernel, edt_z_kernel), none for
// n_fields == 0; in place in fields, no workspace, no atomics; timed from the first launch's start to the last one's end as the
// kernel family of the pending ProfileScope
hipError_t launch_field_from_occupancy(const uint8_t* occupancy, const int (&dims)[3], int n_fields, const edtq::Weights& W,
                                       double limit, double max_distance, bool is_signed, double* fields, hipStream_t stream);
// mrs_tg_field_update_region (mrs_tg_edt_region.hip, mrs_tg_edt_region.hpp): fields holds the field of an earlier occupancy that
// differs from `occupancy` inside the box `plan` was made for (edtq::plan_region) on grid `field` of the stack alone; brings the
// core of the plan up to date, in the full rebuild's bits, and writes no other element.  Three launches (edt_region_x_kernel,
// edt_region_y_kernel, edt_region_z_kernel) through workspace (plan.workspace_doubles doubles, overlapping nothing), or, with
// plan.whole_grid, launch_field_from_occupancy on that one grid without a workspace; timed like it, under the same ProfileScope
hipError_t launch_field_update_region(const uint8_t* occupancy, const int (&dims)[3], int field, const edtq::RegionPlan& plan,
                                      const edtq::Weights& W, double limit, double max_distance, bool is_signed, double* workspace,
                                      double* fields, hipStream_t stream);
// What the rows kernel can do around its solve for the same path, in the same launch:
//   before: the feasibility scaling of the segment times (scaleSegmentTimesWithViolation's T_i <- s_i T_i from the
//           per-segment maxima, written back to seg_times) -- the last stage before the final solve of the Mellinger pipeline;
//   after:  the sampling of the solved trajectory (sampleWholeTrajectory).
// All-null / zero = the plain solve.
struct RowsTail {
  const double* maxima = nullptr;        // [n_segments][9]; with limits and opt_status: scale the times first
  bool maxima_in_launch = false;         // instead: solve at the incoming times, take the maxima of THAT trajectory, scale, solve
                                         // again (the closing stages of a pipeline in one launch; rows_pipeline_applies)
  const double* limits = nullptr;        // [n_paths][9]
  const int32_t* opt_status = nullptr;   // paths whose search was refused (-2) keep their times
  const double* sum_t0 = nullptr;        // [n_paths] total time the outer loop started from: the runaway test (mrs_tg.h)
  double* seg_times_out = nullptr;       // the (scaled) times are written here (the caller's seg_times)
  double sampling_dt = 0.0;              // > 0: sample
  int sample_capacity = 0;
  int32_t* n_samples = nullptr;
  double* samples = nullptr;
  const double* sample_acc = nullptr;    // the walk's accumulated times (sample_acc_table): filled in by launch_solve_rows
  int sample_acc_n = 0;
  const double* pos_wp = nullptr;        // MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: the compact [vertex][4] array the saturated-device
                                         // solve reads vertex positions from (the other kernels read the value array)
};

// A[k] = k additions of dt to 0, the accumulated time of the reference's sampling walk, on the current device: at least
// capacity + 80 entries, built by a kernel on `stream` the first time a (device, dt) pair is seen and ordered behind that
// build for launches on other streams; a bounded, least-recently-used cache (mrs_tg_kernels.hip)
// `pin` keeps the table from being recycled between this call's return and the enqueue of the kernel that reads it (another
// host thread may retire the entry in that window -- a new dt evicting the least recently used one, a larger capacity
// outgrowing it -- and a drain of the retired list would hand the block to someone else): the caller declares an AccPin
// before the call and lets it go out of scope behind its launch.
struct AccPin {
  void* block = nullptr;
  AccPin() = default;
  AccPin(const AccPin&) = delete;
  AccPin& operator=(const AccPin&) = delete;
  ~AccPin();
};
hipError_t sample_acc_table(double dt, int capacity, hipStream_t stream, const double** table_out, int* n_out, AccPin* pin);
void sample_tables_release();  // frees every table (with the last context of the process)

// up to kRowsGroupMax batches of one plan solved by one launch (fixed-times default solve): per batch its arrays
constexpr int kRowsGroupMax = 16;
struct RowsGroup {
  const uint8_t* mask[kRowsGroupMax];
  const double* vals[kRowsGroupMax];
  const double* seg_times[kRowsGroupMax];
  double* coeffs[kRowsGroupMax];
  int32_t* status[kRowsGroupMax];
  double* cost[kRowsGroupMax];
  const double* pos_wp[kRowsGroupMax];  // per batch: waypoints under MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS, else nullptr
  int n = 0;
};

// ---- the fixed-times solve: route first (route_solve, mrs_tg_solve_route.hpp), then a launcher that enqueues what the route says ----
// the operands of a solve, as the kernels take them (device addresses; the optional ones may be null)
struct SolveOperands {
  const uint8_t* mask = nullptr;      // [n_vertices][5]
  const double* vals = nullptr;       // [n_vertices][5][4]
  const double* seg_times = nullptr;  // [n_segments]
  const double* H = nullptr;          // the materialised blocks (a solve that is not fused)
  const double* Ainv = nullptr;
  double* ws = nullptr;               // the global factor store (linear_workspace_doubles): the four- and eight-lane kernels' general
                                      // step, the lane kernel's back substitution
  double* coeffs = nullptr;           // [n_segments][4][10]
  int32_t* status = nullptr;          // [n_paths], optional
  double* cost = nullptr;             // [n_paths], optional
  const int32_t* status_in = nullptr; // [n_paths], optional: the search's status, merged into status
  const double* pos_wp = nullptr;     // MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: the compact [vertex][4] array (SolveRequest::waypoints)
};
// the request of a library call: the hints, the factor store and waypoints as the operands have them, and the compute units
// duo_pays has always counted (of the first device that asked, for the whole process)
int solve_compute_units();
inline SolveRequest solve_request(int d, bool fused, const RouteHints& hints, const SolveOperands& op) {
  SolveRequest q;
  q.derivative = d;
  q.fused = fused;
  q.factor_store = op.ws != nullptr;
  q.waypoints = op.pos_wp != nullptr;
  q.hints = hints;
  q.compute_units = solve_compute_units();
  return q;
}
// Enqueues the single launch `route` describes (its family's launcher below); tail: what rides on the launch -- the route says
// which of it the launch takes (scales, maxima_in_launch, sampling).  A grouped route goes to the group launchers.
hipError_t launch_solve_linear(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream,
                               const RowsTail& tail = RowsTail());
hipError_t launch_solve_tile(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream);
hipError_t launch_solve_rows(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream,
                             const RowsTail& tail = RowsTail());
hipError_t launch_solve_quad(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream,
                             const RowsTail& tail = RowsTail());
// grouped (route.group batches of one plan): g.n must be the route's group.  ws: the plan's factor store, one
// linear_workspace_doubles per batch, for the wavefronts of the four- and eight-lane kernels that take the general masked step
hipError_t launch_solve_rows_group(const BatchView& b, const SolveRoute& route, const RowsGroup& g, hipStream_t stream);
hipError_t launch_solve_quad_group(const BatchView& b, const SolveRoute& route, const RowsGroup& g, double* ws, hipStream_t stream);

}  // namespace mrs_tg

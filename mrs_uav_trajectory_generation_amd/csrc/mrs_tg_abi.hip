// mrs_tg_abi.hip -- implementation of the C ABI declared in include/mrs_tg.h.
// Context / plan bookkeeping, workspace management, host<->device marshalling and the launch
// sequences.  No numerics live here and nothing falls back to the CPU: every failure is reported.
#include <hip/hip_runtime.h>

#include "mrs_tg_pool.h"

#include <algorithm>
#include <thread>
#include <memory>
#include <condition_variable>
#include <atomic>
#include <chrono>
#include <cfloat>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/mrs_tg.h"
#include "mrs_tg_edt.hpp"
#include "mrs_tg_edt_region.hpp"
#include "mrs_tg_fallback.hpp"
#include "mrs_tg_field.hpp"
#include "mrs_tg_pathedit.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_nonlinear.h"
#include "mrs_tg_policy_host.hpp"
#include "../../include/mrs_tg_initial_condition.hpp"

namespace {

std::mutex g_err_mutex;
std::string g_last_error;

void set_global_error(const std::string& s) {
  std::lock_guard<std::mutex> lk(g_err_mutex);
  g_last_error = s;
}

}  // namespace

static std::atomic<int> g_live_contexts{0};

struct mrs_tg_ctx {
  int device = -1;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string last_error;
  bool profiling = false;
  // per-dispatch timing: a ring of event pairs per kernel family, one pair per timed launch (kTimerRing launches can be
  // queued before the oldest is overwritten)
  static constexpr int kTimerRing = 512;
  static constexpr int kTimedKernels = 42;  // kernel_id 0 .. 41 (mrs_tg_last_kernel_ms)
  std::vector<hipEvent_t> ev_start[kTimedKernels], ev_stop[kTimedKernels];
  long long ev_count[kTimedKernels] = {};   // timed launches since profiling was switched on
  hipDeviceProp_t prop;
  double wall_clock_hz = 1.0e8;  // rate of s_memrealtime (hipDeviceAttributeWallClockRate)
  // plan of the most recent mrs_tg_solve_batch: a caller that sends the same batch shape again (the nodelet's
  // deviation loop, a server's fixed batch size) skips the analysis, the uploads and the device allocations
  mrs_tg_plan* cached_plan = nullptr;
  // mrs_tg_solve_batch's transfer arenas, kept across calls and only ever replaced by larger ones: one device block holding
  // every input and output array of a call, and a pinned host block (hipHostMalloc) through which the small host arrays travel
  // packed, one copy each way.  The device block grows behind a synchronise of the stream (StreamIdle; every user of it ends
  // its call with a synchronise, so that one finds an idle stream, and it runs when the block grows, never in a steady-state call)
  mrs_tg::DeviceBlock<char> d_arena;
  mrs_tg::Block<char, mrs_tg::PinnedAlloc> h_arena;
  // pinned host scratch of mrs_tg_optimize_paths (the arrays of its rounds), kept across calls
  mrs_tg::Block<char, mrs_tg::PinnedAlloc> h_scratch;
  // what the most recent mrs_tg_find_trajectory decided (mrs_tg_find_trajectory_info)
  int32_t find_rejection = 0;
  double find_baca_total = 0.0;
};

struct mrs_tg_plan {
  mrs_tg_ctx* ctx = nullptr;
  mrs_tg::BatchView view{};
  std::vector<int32_t> order_host;
  std::vector<int32_t> seg_offsets_host;
  mrs_tg::DeviceBlock<int32_t> d_seg_offsets;  // seg_offsets | order | slot_start in one block (view has the three parts)
  // scratch, allocated on first use; mrs_tg_plan_destroy synchronises and then deletes the plan with its blocks
  mrs_tg::DeviceBlock<double> d_ws;  // grows with what a call needs, behind a synchronise (StreamIdle)
  mrs_tg::DeviceBlock<double> d_H, d_Ainv;  // MRS_TG_FLAG_MATERIALIZED_BLOCKS: both or neither (ensure_both)
  mrs_tg::DeviceBlock<int32_t> d_edit_ws;  // one int32 per vertex: what a path-edit step passes from its first launch to its last
  mrs_tg::NonlinearPlan nl;
};

namespace {

int fail(mrs_tg_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->last_error = buf;
  set_global_error(buf);
  return code;
}

long long budget_ticks(const mrs_tg_ctx* ctx, double seconds_left) {
  // a budget that is already spent still lets every path evaluate its start point once (nlopt checks after an evaluation)
  const double t = seconds_left * ctx->wall_clock_hz;
  return t < 1.0 ? 1ll : (t > 9.0e18 ? (long long)9.0e18 : (long long)t);
}

#define HIP_TRY(ctx, expr)                                                                        \
  do {                                                                                            \
    hipError_t e__ = (expr);                                                                      \
    if (e__ != hipSuccess) return fail((ctx), MRS_TG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

// the two shapes of a state row: the refusal of any other n_orders, or MRS_TG_OK
int check_n_orders(mrs_tg_ctx* ctx, int32_t n_orders) {
  if (n_orders == 1 || n_orders == MRS_TG_STATE_ORDERS) return MRS_TG_OK;
  return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_orders %d is neither 1 (positions and heading) nor %d (all orders)", n_orders,
              MRS_TG_STATE_ORDERS);
}

// What a launcher that stages a whole path in LDS returned, for the caller: hipErrorInvalidValue is its refusal of a path
// that does not fit (mrs_tg::prepare_dynamic_lds)
int staged_launch_result(mrs_tg_ctx* ctx, const mrs_tg_plan* plan, hipError_t e) {
  if (e == hipErrorInvalidValue)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "a path of %d segments needs more than 160 KB of LDS", plan->view.max_segments);
  HIP_TRY(ctx, e);
  return MRS_TG_OK;
}

// Arms the per-dispatch timer for the next timed launch of this thread (the main kernel of the family `kernel_id`):
// the events ride on the kernel launch itself, so their difference is that dispatch's own duration.
struct ProfileScope {
  mrs_tg_ctx* ctx;
  int id;
  bool armed = false;
  ProfileScope(mrs_tg_ctx* c, int kernel_id) : ctx(c), id(kernel_id) {
    if (!ctx->profiling) return;
    if (ctx->ev_start[id].empty()) {
      ctx->ev_start[id].assign(mrs_tg_ctx::kTimerRing, nullptr);
      ctx->ev_stop[id].assign(mrs_tg_ctx::kTimerRing, nullptr);
    }
    const int slot = (int)(ctx->ev_count[id] % mrs_tg_ctx::kTimerRing);
    if (!ctx->ev_start[id][slot]) {
      if (hipEventCreate(&ctx->ev_start[id][slot]) != hipSuccess || hipEventCreate(&ctx->ev_stop[id][slot]) != hipSuccess) return;
    }
    mrs_tg::set_kernel_timer(ctx->ev_start[id][slot], ctx->ev_stop[id][slot]);
    armed = true;
  }
  ~ProfileScope() {
    if (!armed) return;
    const mrs_tg::KernelTimer left = mrs_tg::take_kernel_timer();  // consumed <=> a timed kernel was launched
    if (left.start == nullptr) ++ctx->ev_count[id];
  }
};

// hipSetDevice on every call costs more than asking which device is current
hipError_t use_device(int device) {
  int current = -1;
  if (hipGetDevice(&current) == hipSuccess && current == device) return hipSuccess;  // (another library on this thread may
  return hipSetDevice(device);                                                        // have switched: ask, do not remember)
}

int check_options(mrs_tg_ctx* ctx, const mrs_tg_options* opt) {
  if (!opt) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "options is NULL");
  if (opt->derivative_to_optimize < 0 || opt->derivative_to_optimize > 4)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize %d outside [0, 4]", opt->derivative_to_optimize);
  if (opt->time_alloc_method < MRS_TG_TIME_ALLOC_NONE || opt->time_alloc_method > MRS_TG_TIME_ALLOC_RICHTER_TIME_AND_CONSTRAINTS)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "time_alloc_method %d is not one of -1 (fixed times), 0 / 1 (time only, gradient-free), 2 (Mellinger), "
                "3 / 4 (time and free constraints, gradient-free)",
                opt->time_alloc_method);
  if (opt->sampling_dt > 0 && opt->sample_capacity < 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "negative sample_capacity");
  return MRS_TG_OK;
}

}  // namespace

namespace mrs_tg {
int report_error(mrs_tg_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return fail(ctx, code, "%s", buf);
}
}  // namespace mrs_tg

extern "C" {

int mrs_tg_abi_version(void) { return MRS_TG_ABI_VERSION; }

int mrs_tg_capabilities(void) {
  return (mrs_tg::careful_rerun_built() ? MRS_TG_CAP_CAREFUL_COST : 0) | MRS_TG_CAP_FUTURE_PATHS | MRS_TG_CAP_REFINE |
         MRS_TG_CAP_GRADIENT | MRS_TG_CAP_MAXIMA_GRADIENT | MRS_TG_CAP_SAMPLE_GRADIENT | MRS_TG_CAP_EVALUATE | MRS_TG_CAP_DEVIATION |
         MRS_TG_CAP_ESTIMATE_GRADIENT | MRS_TG_CAP_WAYPOINT_PASSAGE | MRS_TG_CAP_BACA | MRS_TG_CAP_FALLBACK_SAMPLE |
         MRS_TG_CAP_PATH_EDIT | MRS_TG_CAP_TRAVEL_HEADING | MRS_TG_CAP_INITIAL_CONDITION | MRS_TG_CAP_REQUEST |
         MRS_TG_CAP_MUTUAL_CLEARANCE | MRS_TG_CAP_OBSTACLE_CLEARANCE | MRS_TG_CAP_FIELD_CLEARANCE |
         MRS_TG_CAP_FIELD_FROM_OCCUPANCY | MRS_TG_CAP_FIELD_UPDATE_REGION;
}

// prepareInitialCondition (:506-614) + the first-waypoint rule (:650-655): mrs_tg_initial_condition.hpp, host arithmetic
int mrs_tg_prepare_initial_condition(const mrs_tg_waypoint* tracker_pose, const mrs_tg_initial_state* tracker_state,
                                     double tracker_age_s, const mrs_tg_prediction* prediction, const double* uav_pose4,
                                     double takeoff_height, double path_time_offset_s, int32_t n_path_waypoints,
                                     int32_t dont_prepend, mrs_tg_waypoint* initial_waypoint_out,
                                     mrs_tg_initial_state* initial_state_out, int32_t* has_initial_condition_out,
                                     int32_t* from_future_out, int32_t* sample_offset_out, int32_t* drop_first_waypoint_out) {
  if (!initial_waypoint_out || !initial_state_out || !has_initial_condition_out || !from_future_out || !sample_offset_out ||
      !drop_first_waypoint_out)
    return mrs_tg::report_error(nullptr, MRS_TG_ERR_INVALID_ARG, "mrs_tg_prepare_initial_condition: every output is required");
  mrs_tg::initial_condition::Decision d;
  const char* why = "";
  const int rc = mrs_tg::initial_condition::prepare(tracker_pose, tracker_state, tracker_age_s, prediction, uav_pose4, takeoff_height,
                                                    path_time_offset_s, n_path_waypoints, dont_prepend != 0, &d, &why);
  if (rc != MRS_TG_OK) return mrs_tg::report_error(nullptr, rc, "mrs_tg_prepare_initial_condition: %s", why);
  *initial_waypoint_out = d.waypoint;
  *initial_state_out = d.state;
  *has_initial_condition_out = d.has_initial_condition ? 1 : 0;
  *from_future_out = d.from_future ? 1 : 0;
  *sample_offset_out = d.sample_offset;
  *drop_first_waypoint_out = d.drop_first_waypoint ? 1 : 0;
  return MRS_TG_OK;
}

// the pre-trajectory of a path from the future (:801-838)
int32_t mrs_tg_splice_prediction(const mrs_tg_prediction* prediction, int32_t sample_offset, double prediction_age_s,
                                 double* samples, int32_t n_samples, int32_t sample_capacity) {
  const char* why = "";
  const int32_t n = mrs_tg::initial_condition::splice(prediction, sample_offset, prediction_age_s, samples, n_samples,
                                                      sample_capacity, &why);
  if (n < 0) return mrs_tg::report_error(nullptr, n, "mrs_tg_splice_prediction: %s", why);
  return n;
}

void mrs_tg_kernel_trace_reset(void) { mrs_tg::kernel_trace_reset(); }

int mrs_tg_kernel_trace(const char** names_out, int capacity) {
  if (!names_out || capacity <= 0) return 0;
  return mrs_tg::kernel_trace(names_out, capacity);
}

void mrs_tg_default_options(mrs_tg_options* opt) {
  if (!opt) return;
  mrs_tg::policy::default_solver_options(opt);
}

const char* mrs_tg_last_error(const mrs_tg_ctx* ctx) {
  if (ctx) return ctx->last_error.c_str();
  static thread_local std::string copy;
  std::lock_guard<std::mutex> lk(g_err_mutex);
  copy = g_last_error;
  return copy.c_str();
}

int mrs_tg_create(int device_ordinal, mrs_tg_ctx** ctx_out) {
  if (!ctx_out) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx_out is NULL");
  *ctx_out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, MRS_TG_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device_ordinal < 0 || device_ordinal >= n)
    return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "device ordinal %d outside [0, %d)", device_ordinal, n);
  mrs_tg_ctx* ctx = new (std::nothrow) mrs_tg_ctx();
  if (!ctx) return fail(nullptr, MRS_TG_ERR_NOMEM, "out of host memory");
  ctx->device = device_ordinal;
  if ((e = use_device(device_ordinal)) != hipSuccess || (e = hipGetDeviceProperties(&ctx->prop, device_ordinal)) != hipSuccess ||
      (e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
    delete ctx;
    return fail(nullptr, MRS_TG_ERR_HIP, "device setup failed: %s", hipGetErrorString(e));
  }
  ctx->stream = ctx->own_stream;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_ordinal) == hipSuccess && khz > 0)
      ctx->wall_clock_hz = 1.0e3 * (double)khz;
  }
  ++g_live_contexts;
  *ctx_out = ctx;
  return MRS_TG_OK;
}

void mrs_tg_destroy(mrs_tg_ctx* ctx) {
  if (!ctx) return;
  (void)use_device(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->cached_plan) {
    mrs_tg_plan* p = ctx->cached_plan;
    ctx->cached_plan = nullptr;
    mrs_tg_plan_destroy(p);
  }
  for (int i = 0; i < mrs_tg_ctx::kTimedKernels; ++i) {
    for (hipEvent_t e : ctx->ev_start[i])
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_stop[i])
      if (e) (void)hipEventDestroy(e);
  }
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  if (--g_live_contexts == 0) {  // the sampling tables and the cached device blocks go with the last context
    mrs_tg::sample_tables_release();
    mrs_tg::pool_release_cached();
  }
}

int mrs_tg_set_stream(mrs_tg_ctx* ctx, void* hip_stream) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return MRS_TG_OK;
}

int mrs_tg_reset_stream(mrs_tg_ctx* ctx) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  ctx->stream = ctx->own_stream;
  return MRS_TG_OK;
}

int mrs_tg_synchronize(mrs_tg_ctx* ctx) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_set_profiling(mrs_tg_ctx* ctx, int enabled) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  ctx->profiling = enabled != 0;
  if (ctx->profiling)
    for (int i = 0; i < mrs_tg_ctx::kTimedKernels; ++i) ctx->ev_count[i] = 0;  // a new series
  return MRS_TG_OK;
}

int mrs_tg_kernel_ms_history(mrs_tg_ctx* ctx, int kernel_id, float* ms_out, int capacity) {
  if (!ctx || (capacity > 0 && !ms_out)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  if (kernel_id < 0 || kernel_id >= mrs_tg_ctx::kTimedKernels)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "kernel id %d outside [0, %d]", kernel_id, mrs_tg_ctx::kTimedKernels - 1);
  const long long total = ctx->ev_count[kernel_id];
  long long n = total < mrs_tg_ctx::kTimerRing ? total : mrs_tg_ctx::kTimerRing;
  if (n > capacity) n = capacity;
  HIP_TRY(ctx, use_device(ctx->device));
  for (long long i = 0; i < n; ++i) {  // the newest n launches, oldest first
    const int slot = (int)((total - n + i) % mrs_tg_ctx::kTimerRing);
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_stop[kernel_id][slot]));
    HIP_TRY(ctx, hipEventElapsedTime(&ms_out[i], ctx->ev_start[kernel_id][slot], ctx->ev_stop[kernel_id][slot]));
  }
  return (int)n;
}

int mrs_tg_last_kernel_ms(mrs_tg_ctx* ctx, int kernel_id, float* ms_out) {
  if (!ctx || !ms_out) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  if (kernel_id < 0 || kernel_id >= mrs_tg_ctx::kTimedKernels || ctx->ev_count[kernel_id] == 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "no timed launch recorded for kernel id %d (mrs_tg_set_profiling, then a call that runs that kernel)", kernel_id);
  const int n = mrs_tg_kernel_ms_history(ctx, kernel_id, ms_out, 1);
  return n == 1 ? MRS_TG_OK : n;
}

// ---- plan ------------------------------------------------------------------------------------

int mrs_tg_plan_create(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* so, mrs_tg_plan** plan_out) {
  if (!ctx || !plan_out || !so) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  *plan_out = nullptr;
  if (n_paths < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "negative n_paths");
  if (so[0] != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "seg_offsets[0] must be 0");
  int max_S = 0, min_S = n_paths ? INT32_MAX : 0;
  for (int p = 0; p < n_paths; ++p) {
    const int S = so[p + 1] - so[p];
    if (S < 1) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "path %d has %d segments (need >= 1)", p, S);
    if (S > MRS_TG_MAX_SEGMENTS)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "path %d has %d segments (at most %d)", p, S, MRS_TG_MAX_SEGMENTS);
    max_S = std::max(max_S, S);
    min_S = std::min(min_S, S);
  }
  HIP_TRY(ctx, use_device(ctx->device));
  mrs_tg_plan* plan = new (std::nothrow) mrs_tg_plan();
  if (!plan) return fail(ctx, MRS_TG_ERR_NOMEM, "out of host memory");
  plan->ctx = ctx;
  plan->seg_offsets_host.assign(so, so + n_paths + 1);
  plan->order_host.resize(n_paths);
  std::iota(plan->order_host.begin(), plan->order_host.end(), 0);
  std::stable_sort(plan->order_host.begin(), plan->order_host.end(),
                   [so](int a, int b) { return (so[a + 1] - so[a]) > (so[b + 1] - so[b]); });
  // slot_start[j] = number of (q, j') pairs with j' < j; paths sorted longest first => slot j is a prefix
  std::vector<int32_t> slot_start(max_S + 1, 0);
  {
    std::vector<int32_t> cnt(max_S + 1, 0);
    for (int p = 0; p < n_paths; ++p) cnt[so[p + 1] - so[p]]++;  // paths with exactly S segments
    int longer = 0;                                              // paths with S > j
    std::vector<int32_t> per_slot(max_S, 0);
    for (int j = max_S - 1; j >= 0; --j) {
      longer += cnt[j + 1];
      per_slot[j] = longer;
    }
    for (int j = 0; j < max_S; ++j) slot_start[j + 1] = slot_start[j] + per_slot[j];
  }
  auto cleanup = [&](int code) {
    mrs_tg_plan_destroy(plan);
    return code;
  };
  // the three structure arrays in ONE device block, uploaded by one copy (a blocking copy costs the host 10-20 us whatever its
  // size, and the nodelet's deviation loop makes a plan per round: three of them were a tenth of a one-request call)
  hipError_t e;
  std::vector<int32_t> packed;
  packed.reserve((size_t)n_paths * 2 + 2 + (size_t)max_S + 1);
  packed.insert(packed.end(), so, so + n_paths + 1);
  const size_t off_order = packed.size();
  packed.insert(packed.end(), plan->order_host.begin(), plan->order_host.end());
  if (n_paths == 0) packed.push_back(0);
  const size_t off_slot = packed.size();
  packed.insert(packed.end(), slot_start.begin(), slot_start.end());
  if ((e = plan->d_seg_offsets.ensure(packed.size())) != hipSuccess ||
      (e = hipMemcpy(plan->d_seg_offsets.get(), packed.data(), sizeof(int32_t) * packed.size(), hipMemcpyHostToDevice)) !=
          hipSuccess)
    return cleanup(fail(ctx, MRS_TG_ERR_HIP, "plan allocation failed: %s", hipGetErrorString(e)));
  plan->view.n_paths = n_paths;
  plan->view.n_segments = so[n_paths];
  plan->view.max_segments = max_S;
  plan->view.uniform_S = (n_paths > 0 && min_S == max_S) ? max_S : 0;
  plan->view.seg_offsets = plan->d_seg_offsets.get();
  plan->view.order = plan->view.seg_offsets + off_order;  // (views into the one block)
  plan->view.slot_start = plan->view.seg_offsets + off_slot;
  plan->nl.host = mrs_tg::nonlinear_host_plan(plan->seg_offsets_host, plan->order_host);
  *plan_out = plan;
  return MRS_TG_OK;
}

void mrs_tg_plan_destroy(mrs_tg_plan* plan) {
  if (!plan) return;
  (void)use_device(plan->ctx->device);
  (void)hipStreamSynchronize(plan->ctx->stream);
  delete plan;  // its blocks go back to the pool behind the synchronise above
}

int32_t mrs_tg_plan_n_paths(const mrs_tg_plan* plan) { return plan ? plan->view.n_paths : 0; }
int32_t mrs_tg_plan_n_segments(const mrs_tg_plan* plan) { return plan ? plan->view.n_segments : 0; }
int32_t mrs_tg_plan_max_segments(const mrs_tg_plan* plan) { return plan ? plan->view.max_segments : 0; }

int mrs_tg_plan_get_order(const mrs_tg_plan* plan, int32_t* order_out) {
  if (!plan || !order_out) return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  std::copy(plan->order_host.begin(), plan->order_host.end(), order_out);
  return MRS_TG_OK;
}

size_t mrs_tg_plan_block_bytes(const mrs_tg_plan* plan) {
  if (!plan) return 0;
  return (size_t)plan->view.max_segments * 100 * (size_t)plan->view.n_paths * sizeof(double);
}

int mrs_tg_plan_assemble(mrs_tg_plan* plan, int32_t d, const double* seg_times_dev, double* H_dev, double* Ainv_dev) {
  if (!plan || !seg_times_dev || !H_dev || !Ainv_dev)
    return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  if (d < 0 || d > 4) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize %d outside [0, 4]", d);
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 0);
  HIP_TRY(ctx, mrs_tg::launch_assemble(plan->view, d, seg_times_dev, H_dev, Ainv_dev, ctx->stream));
  return MRS_TG_OK;
}

// mrs_tg_plan_solve, for every entry point that ends in it.  moving_start_seen: the caller has the first vertices in host
// memory and saw one that moves (mrs_tg_solve_batch, the policy's device round); a device-resident caller cannot say
static int plan_solve(mrs_tg_plan* plan, const double* wp, const uint8_t* mask, const double* vals, const double* limits,
                      const mrs_tg_options* opt, double* seg_times, double* coeffs, int32_t* status, double* cost,
                      int32_t* n_samples, double* samples, bool moving_start_seen) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  int rc = check_options(ctx, opt);
  if (rc != MRS_TG_OK) return rc;
  if (!mask || !vals || !seg_times || !coeffs || !status)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "fixed_mask, fixed_values, seg_times, coeffs_out and status_out are required");
  if ((opt->estimate_times || opt->time_alloc_method != MRS_TG_TIME_ALLOC_NONE) && !limits)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "limits are required for time estimation and for every time-allocation mode");
  if (opt->estimate_times && !wp) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints are required when estimate_times is set");
  if ((opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) && !wp)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS needs the waypoints array");
  if (opt->sampling_dt > 0 && !n_samples) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_samples_out is required when sampling");
  HIP_TRY(ctx, use_device(ctx->device));
  const mrs_tg::BatchView& b = plan->view;
  // MRS_TG_VERIFY_FLAGS=1 (debug / test knob, read once): the statement of MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS is checked on
  // every solve, not only at bind time -- a blocking check; a false statement fails the call instead of solving the
  // waypoints' problem on launches that take the saturated-device kernel and the caller's on the others
  if (mrs_tg::knob::verify_flags() && !mrs_tg::dry_run() && (opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS)) {
    long long bad = 0;
    HIP_TRY(ctx, mrs_tg::count_position_mismatches(b, wp, mask, vals, ctx->stream, &bad));
    if (bad != 0)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                  "MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: %lld vertices whose position constraint is absent or differs from their waypoint",
                  bad);
  }
  const double* pos_wp = (opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) ? wp : nullptr;
  const int d = opt->derivative_to_optimize;
  const mrs_tg::RouteHints hints =
      mrs_tg::route_hints(opt->flags, moving_start_seen, opt->time_alloc_method, (size_t)b.n_paths, b.max_segments);
  bool sampled = false;  // the sampling rode on the final solve's launch
  // MRS_TG_FLAG_REFINE: the refinement pass follows the final solve, so no sampling rides on a solve launch -- the solves go
  // out exactly as in the same call without sampling, and the sampler reads the refined coefficients
  const bool refine = (opt->flags & MRS_TG_FLAG_REFINE) != 0;
  const double solve_sampling_dt = refine ? 0.0 : opt->sampling_dt;
  // (the Mellinger pipeline takes the estimate as its start point itself: mrs_tg::NonlinearParams::estimate_wp)
  if (opt->estimate_times && opt->time_alloc_method != MRS_TG_TIME_ALLOC_MELLINGER)
    HIP_TRY(ctx, mrs_tg::launch_estimate_times(b, wp, limits, seg_times, ctx->stream));

  if (opt->time_alloc_method != MRS_TG_TIME_ALLOC_NONE && opt->time_alloc_method != MRS_TG_TIME_ALLOC_MELLINGER) {
    mrs_tg::DfoParams prm;
    prm.derivative = d;
    prm.mode = opt->time_alloc_method;
    prm.max_iterations = opt->max_iterations;
    prm.f_rel = opt->f_rel;
    prm.f_abs = opt->f_abs;
    prm.x_rel = opt->x_rel;
    prm.x_abs = opt->x_abs;
    prm.time_penalty = opt->time_penalty;
    prm.soft_weight = opt->soft_constraint_weight;
    prm.use_soft = opt->use_soft_constraints;
    prm.initial_stepsize_rel = opt->initial_stepsize_rel;
    prm.time_budget_ticks = opt->max_time_s > 0 ? budget_ticks(ctx, opt->max_time_s) : 0;
    ProfileScope ps(ctx, 2);
    HIP_TRY(ctx, mrs_tg::launch_dfo(plan->nl, b, hints, prm, mask, vals, limits, seg_times, coeffs, status, cost, ctx->stream,
                                    (opt->flags & MRS_TG_FLAG_GENERAL_PATTERNS) != 0));
  } else if (opt->time_alloc_method == MRS_TG_TIME_ALLOC_MELLINGER) {
    mrs_tg::NonlinearParams prm;
    prm.derivative = d;
    prm.max_iterations = opt->max_iterations;
    prm.f_rel = opt->f_rel;
    prm.f_abs = opt->f_abs;
    prm.x_rel = opt->x_rel;
    prm.x_abs = opt->x_abs;
    prm.time_budget_ticks = opt->max_time_s > 0 ? budget_ticks(ctx, opt->max_time_s) : 0;
    if ((opt->flags & MRS_TG_FLAG_CAREFUL_COST) && !mrs_tg::careful_rerun_built())
      return fail(ctx, MRS_TG_ERR_UNSUPPORTED,
                  "MRS_TG_FLAG_CAREFUL_COST: this library was built without the careful re-run (rebuild with -DMRS_TG_WITH_CAREFUL=1)");
    prm.careful_cap = (opt->flags & MRS_TG_FLAG_CAREFUL_COST) ? 1 : 0;
    if (opt->estimate_times) {
      prm.estimate_wp = wp;
      prm.estimate_limits = limits;
    }
    prm.pos_wp = pos_wp;
    prm.reference_status = (opt->flags & MRS_TG_FLAG_REFERENCE_STATUS) != 0;
    ProfileScope ps(ctx, 2);
    HIP_TRY(ctx, mrs_tg::launch_nonlinear(plan->nl, b, hints, prm, mask, vals, limits, seg_times, coeffs, status, cost,
                                          ctx->stream, solve_sampling_dt, opt->sample_capacity, n_samples, samples, &sampled,
                                          (opt->flags & MRS_TG_FLAG_GENERAL_PATTERNS) != 0));
  } else {
    const bool fused = (opt->flags & MRS_TG_FLAG_MATERIALIZED_BLOCKS) == 0;  // the default since ABI 2
    const bool general = (opt->flags & MRS_TG_FLAG_GENERAL_PATTERNS) != 0;   // position-free vertices may occur
    HIP_TRY(ctx, plan->d_ws.ensure(general ? std::max(mrs_tg::linear_workspace_doubles(b), mrs_tg::general_workspace_doubles(b))
                                           : mrs_tg::linear_workspace_doubles(b),
                                   mrs_tg::StreamIdle{ctx->stream}));
    if (!fused) {
      const size_t block_doubles = mrs_tg_plan_block_bytes(plan) / sizeof(double);
      HIP_TRY(ctx, mrs_tg::ensure_both(plan->d_H, block_doubles, plan->d_Ainv, block_doubles));
      ProfileScope ps(ctx, 0);
      HIP_TRY(ctx, mrs_tg::launch_assemble(b, d, seg_times, plan->d_H.get(), plan->d_Ainv.get(), ctx->stream));
    }
    ProfileScope ps(ctx, 1);
    mrs_tg::SolveOperands op;
    op.mask = mask;
    op.vals = vals;
    op.seg_times = seg_times;
    op.H = plan->d_H.get();
    op.Ainv = plan->d_Ainv.get();
    op.ws = plan->d_ws.get();
    op.coeffs = coeffs;
    op.status = status;
    op.cost = cost;
    op.pos_wp = general ? nullptr : pos_wp;
    mrs_tg::SolveRequest request = mrs_tg::solve_request(d, fused, hints, op);
    request.sampling = solve_sampling_dt > 0 && !general;  // solve and sample in one launch, where the route takes it
    const mrs_tg::SolveRoute route = mrs_tg::route_solve(b, request);
    mrs_tg::RowsTail tail;
    if (route.sampling) {
      tail.sampling_dt = opt->sampling_dt;
      tail.sample_capacity = opt->sample_capacity;
      tail.n_samples = n_samples;
      tail.samples = samples;
    }
    HIP_TRY(ctx, mrs_tg::launch_solve_linear(b, route, op, ctx->stream, tail));
    sampled = route.sampling;
    // the paths the fast kernels sent back with status -2 (a vertex without a position constraint): 5 x 5 vertex blocks
    if (general)
      HIP_TRY(ctx, mrs_tg::launch_solve_general(b, d, mask, vals, seg_times, plan->d_ws.get(), coeffs, status, cost, ctx->stream));
  }
  if (refine) {  // every mode's final solve: the paths with status > 0 at the returned times (the dry run allocates nothing)
    if (!mrs_tg::dry_run()) HIP_TRY(ctx, plan->d_ws.ensure(mrs_tg::refine_workspace_doubles(b), mrs_tg::StreamIdle{ctx->stream}));
    HIP_TRY(ctx, mrs_tg::launch_refine(b, d, mask, vals, seg_times, plan->d_ws.get(), coeffs, status, cost, ctx->stream));
  }
  if (opt->sampling_dt > 0 && !sampled)
    HIP_TRY(ctx, mrs_tg::launch_sample(b, coeffs, seg_times, opt->sampling_dt, opt->sample_capacity, n_samples, samples,
                                       ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_solve(mrs_tg_plan* plan, const double* wp, const uint8_t* mask, const double* vals, const double* limits,
                      const mrs_tg_options* opt, double* seg_times, double* coeffs, int32_t* status, double* cost,
                      int32_t* n_samples, double* samples) {
  return plan_solve(plan, wp, mask, vals, limits, opt, seg_times, coeffs, status, cost, n_samples, samples, false);
}

static constexpr size_t kGroupWsPresizeBytes = (size_t)256 << 20;  // bind-time reservation of a grouped launch's factor stores

// the route of a grouped dispatch of `group` batches of one plan (the plan's factor store is grown for it where it needs one)
static mrs_tg::SolveRoute group_route(const mrs_tg::BatchView& b, int d, const mrs_tg::RouteHints& hints, int group, bool waypoints) {
  mrs_tg::SolveRequest request;
  request.derivative = d;
  request.group = group;
  request.waypoints = waypoints;
  request.hints = hints;
  request.compute_units = mrs_tg::solve_compute_units();
  return mrs_tg::route_solve(b, request);
}

struct mrs_tg_bound_solve {
  mrs_tg_plan* plan;
  const double* wp;
  const uint8_t* mask;
  const double* vals;
  const double* limits;
  mrs_tg_options opt;
  double* seg_times;
  double* coeffs;
  int32_t* status;
  double* cost;
  int32_t* n_samples;
  double* samples;
};

int mrs_tg_plan_bind_solve(mrs_tg_plan* plan, const double* wp, const uint8_t* mask, const double* vals, const double* limits,
                           const mrs_tg_options* opt, double* seg_times, double* coeffs, int32_t* status, double* cost,
                           int32_t* n_samples, double* samples, mrs_tg_bound_solve** bound_out) {
  if (!plan || !bound_out) return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  *bound_out = nullptr;
  const int rc = check_options(plan->ctx, opt);
  if (rc != MRS_TG_OK) return rc;
  if (opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) {
    // the caller's statement, checked once on the arrays as they are now (a blocking check: binding is not a hot path)
    if (!wp || !mask || !vals) return fail(plan->ctx, MRS_TG_ERR_INVALID_ARG, "MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS needs waypoints, fixed_mask and fixed_values");
    mrs_tg_ctx* ctx = plan->ctx;
    HIP_TRY(ctx, use_device(ctx->device));
    long long bad = 0;
    HIP_TRY(ctx, mrs_tg::count_position_mismatches(plan->view, wp, mask, vals, ctx->stream, &bad));
    if (bad != 0)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                  "MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: %lld vertices whose position constraint is absent or differs from their waypoint",
                  bad);
  }
  // A fixed-times default solve can go out in grouped launches (mrs_tg_bound_solve_launch_group), whose saturated-device kernel
  // wants one factor store per batch of the group for paths that need the general step.  SMALL plans reserve it HERE, once,
  // so that the first large group does not pay an allocation and a stream synchronisation inside somebody's timed region;
  // a plan whose full group would hold more than kGroupWsPresizeBytes (1024 x 10: 157 MB for 16 batches; 8192 x 10 would
  // be 1.26 GB, 65536 x 10 ten) reserves nothing at bind time -- most bound solves are never launched in a group -- and
  // mrs_tg_bound_solve_launch_group sizes the store for the group it actually launches.
  if (opt->time_alloc_method == MRS_TG_TIME_ALLOC_NONE && !opt->estimate_times && opt->sampling_dt <= 0 &&
      !(opt->flags & (MRS_TG_FLAG_MATERIALIZED_BLOCKS | MRS_TG_FLAG_GENERAL_PATTERNS)) &&
      mrs_tg::uses_factor_store(group_route(plan->view, opt->derivative_to_optimize, mrs_tg::RouteHints{}, mrs_tg::kRowsGroupMax, false)) &&
      (size_t)mrs_tg::kRowsGroupMax * mrs_tg::linear_workspace_doubles(plan->view) * sizeof(double) <= kGroupWsPresizeBytes) {
    HIP_TRY(plan->ctx, plan->d_ws.ensure((size_t)mrs_tg::kRowsGroupMax * mrs_tg::linear_workspace_doubles(plan->view),
                                         mrs_tg::StreamIdle{plan->ctx->stream}));
  }
  mrs_tg_bound_solve* b = new (std::nothrow) mrs_tg_bound_solve{plan, wp, mask, vals, limits, *opt, seg_times, coeffs, status, cost,
                                                                n_samples, samples};
  if (!b) return fail(plan->ctx, MRS_TG_ERR_NOMEM, "out of host memory");
  *bound_out = b;
  return MRS_TG_OK;
}

int mrs_tg_bound_solve_launch(mrs_tg_bound_solve* b) {
  if (!b) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solve is NULL");
  return mrs_tg_plan_solve(b->plan, b->wp, b->mask, b->vals, b->limits, &b->opt, b->seg_times, b->coeffs, b->status, b->cost,
                           b->n_samples, b->samples);
}

void mrs_tg_bound_solve_destroy(mrs_tg_bound_solve* b) { delete b; }

// ---- the issue loop on several host threads ------------------------------------------------------
// One runtime launch costs the host 3.5-4.5 us; four 10 us kernels in flight retire one every 2.6 us, so a single issuing
// thread is what bounds a host that keeps four batches in flight.  Helper threads (created on first use, one per extra
// issuing thread) take the launches of the bound solves k = j, j + T, ... -- the order within a bound solve's stream is kept,
// the streams are independent anyway.  A helper spins for work for kSpinUs after its last job (a server that issues runs
// back to back never pays a wake-up), then sleeps on a condition variable.
namespace {

struct IssueJob {
  mrs_tg_bound_solve* const* bound = nullptr;
  int n_bound = 0, n_launches = 0, me = 0;
  const int* owner = nullptr;  // [n_bound] the thread that issues bound solve i: solves that share a context share a thread
  int rc = MRS_TG_OK;
};

class IssuePool {
 public:
  static IssuePool& instance() {
    static IssuePool pool;
    return pool;
  }
  // runs jobs[1..] on helpers and jobs[0] on the caller; returns when all are done
  void run(std::vector<IssueJob>& jobs) {
    std::lock_guard<std::mutex> one_caller(run_mutex_);  // the workers and their job slots serve one run at a time
    const int helpers = (int)jobs.size() - 1;
    ensure(helpers);
    for (int j = 0; j < helpers; ++j) workers_[j]->post(&jobs[j + 1]);
    issue(jobs[0]);
    for (int j = 0; j < helpers; ++j) workers_[j]->wait();
  }
  static void issue(IssueJob& job) {
    for (int k = 0, i = 0; k < job.n_launches; ++k, i = (i + 1 == job.n_bound) ? 0 : i + 1) {
      if (job.owner[i] != job.me) continue;
      const int rc = mrs_tg_bound_solve_launch(job.bound[i]);
      if (rc != MRS_TG_OK) {
        job.rc = rc;
        return;
      }
    }
  }

 private:
  static constexpr int kSpinUs = 2000;
  struct Worker {
    std::atomic<IssueJob*> job{nullptr};
    std::atomic<bool> done{true}, quit{false};
    std::mutex m;
    std::condition_variable cv;
    std::thread th;
    Worker() : th([this] { loop(); }) {}
    ~Worker() {
      quit.store(true);
      {
        std::lock_guard<std::mutex> lk(m);
      }
      cv.notify_one();
      th.join();
    }
    void post(IssueJob* j) {
      done.store(false, std::memory_order_relaxed);
      job.store(j, std::memory_order_release);
      {
        std::lock_guard<std::mutex> lk(m);  // pairs with the sleeper's predicate check
      }
      cv.notify_one();
    }
    void wait() {
      while (!done.load(std::memory_order_acquire)) __builtin_ia32_pause();
    }
    void loop() {
      while (!quit.load()) {
        IssueJob* j = nullptr;
        const auto t_end = std::chrono::steady_clock::now() + std::chrono::microseconds(kSpinUs);
        while (!(j = job.exchange(nullptr, std::memory_order_acquire))) {
          if (quit.load()) return;
          if (std::chrono::steady_clock::now() > t_end) {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [this] { return job.load(std::memory_order_acquire) != nullptr || quit.load(); });
          } else {
            __builtin_ia32_pause();
          }
        }
        IssuePool::issue(*j);
        done.store(true, std::memory_order_release);
      }
    }
  };
  void ensure(int helpers) {
    while ((int)workers_.size() < helpers) workers_.emplace_back(new Worker());
  }
  std::vector<std::unique_ptr<Worker>> workers_;
  std::mutex run_mutex_;
};

}  // namespace

int mrs_tg_bound_solve_launch_many_mt(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches,
                                      int32_t n_threads) {
  if (!bound || n_bound < 1 || n_launches < 0) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solves are required");
  for (int32_t i = 0; i < n_bound; ++i)
    if (!bound[i]) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solve %d is NULL", i);
  try {
    // A context (its plans' workspaces, its timers, its error string) is driven by one thread at a time: the bound solves
    // are partitioned by CONTEXT, not by index -- every solve of a context goes to the same issuing thread, and the
    // number of threads is at most the number of distinct contexts.
    std::vector<mrs_tg_ctx*> ctxs;
    std::vector<int> owner((size_t)n_bound);
    for (int32_t i = 0; i < n_bound; ++i) {
      mrs_tg_ctx* c = bound[i]->plan->ctx;
      size_t j = 0;
      while (j < ctxs.size() && ctxs[j] != c) ++j;
      if (j == ctxs.size()) ctxs.push_back(c);
      owner[(size_t)i] = (int)j;
    }
    int T = n_threads < 1 ? 1 : n_threads;
    if (T > (int)ctxs.size()) T = (int)ctxs.size();
    if (T > 8) T = 8;
    if (T == 1) return mrs_tg_bound_solve_launch_many(bound, n_bound, n_launches);
    for (int& o : owner) o %= T;
    std::vector<IssueJob> jobs((size_t)T);
    for (int j = 0; j < T; ++j) {
      jobs[j].bound = bound;
      jobs[j].n_bound = n_bound;
      jobs[j].n_launches = n_launches;
      jobs[j].me = j;
      jobs[j].owner = owner.data();
    }
    IssuePool::instance().run(jobs);
    for (const IssueJob& j : jobs)
      if (j.rc != MRS_TG_OK) return j.rc;
    return MRS_TG_OK;
  } catch (const std::bad_alloc&) {
    return fail(nullptr, MRS_TG_ERR_NOMEM, "out of host memory");
  } catch (const std::exception& ex) {  // std::system_error of a thread that could not be started: nothing crosses the C boundary
    return fail(nullptr, MRS_TG_ERR_UNSUPPORTED, "issue threads: %s", ex.what());
  }
}

int mrs_tg_bound_solve_launch_many(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches) {
  if (!bound || n_bound < 1 || n_launches < 0) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solves are required");
  for (int32_t i = 0; i < n_bound; ++i)
    if (!bound[i]) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solve %d is NULL", i);
  for (int32_t k = 0, i = 0; k < n_launches; ++k, i = (i + 1 == n_bound) ? 0 : i + 1) {
    const int rc = mrs_tg_bound_solve_launch(bound[i]);
    if (rc != MRS_TG_OK) return rc;
  }
  return MRS_TG_OK;
}

// The issue loop with consecutive launches packed into one dispatch: launch k still solves bound[k % n_bound], but a run of
// consecutive launches whose bound solves share a PLAN (one batch structure, one context and stream; the solves differ in
// their input / output arrays) goes out as a single kernel whose workgroups are divided among the batches, on that plan's
// stream.  bound = [A0, A1, B0, B1] with A*, B* on two plans therefore issues (A0 A1), (B0 B1), (A0 A1), ... alternately on
// the two streams.  Fixed times, the default solve, no sampling.  Every path runs the single-batch kernel's instructions.
int mrs_tg_bound_solve_launch_group(mrs_tg_bound_solve* const* bound, int32_t n_bound, int32_t n_launches) {
  if (!bound || n_bound < 1 || n_launches < 0) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solves are required");
  for (int32_t i = 0; i < n_bound; ++i)
    if (!bound[i]) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "bound solve %d is NULL", i);
  for (int32_t i = 0; i < n_bound; ++i) {
    const mrs_tg_bound_solve* b = bound[i];
    mrs_tg_ctx* ctx = b->plan->ctx;
    const mrs_tg_options& o = b->opt;
    if (o.flags & MRS_TG_FLAG_REFINE)
      return fail(ctx, MRS_TG_ERR_UNSUPPORTED, "grouped launches do not take MRS_TG_FLAG_REFINE (solve %d sets it)", i);
    if (o.time_alloc_method != MRS_TG_TIME_ALLOC_NONE || o.estimate_times || o.sampling_dt > 0 ||
        (o.flags & (MRS_TG_FLAG_MATERIALIZED_BLOCKS | MRS_TG_FLAG_GENERAL_PATTERNS)))
      return fail(ctx, MRS_TG_ERR_UNSUPPORTED, "grouped launches are for the fixed-times default solve without sampling (solve %d differs)", i);
    if (!b->mask || !b->vals || !b->seg_times || !b->coeffs || !b->status)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "fixed_mask, fixed_values, seg_times, coeffs_out and status_out are required (solve %d)", i);
    if (!mrs_tg::rows_kernel_applies(b->plan->view, false))
      return fail(ctx, MRS_TG_ERR_UNSUPPORTED, "grouped launches need a batch the one-lane-per-unknown solve takes (solve %d: paths too long)", i);
  }
  for (int32_t k = 0; k < n_launches;) {
    const mrs_tg_bound_solve* first = bound[k % n_bound];
    mrs_tg_plan* plan = first->plan;
    mrs_tg_ctx* ctx = plan->ctx;
    mrs_tg::RowsGroup g;
    mrs_tg::RouteHints hints;  // (of the dispatch: the batches' other hints have no say in a grouped launch)
    bool waypoints = true;     // every batch of the group states that its positions are its waypoints
    for (; g.n < mrs_tg::kRowsGroupMax && k < n_launches; ++k, ++g.n) {
      const mrs_tg_bound_solve* b = bound[k % n_bound];
      if (b->plan != plan || b->opt.derivative_to_optimize != first->opt.derivative_to_optimize) break;
      if (g.n > 0 && b == first) break;  // the round is complete: the same arrays twice in one launch would be written twice
      g.mask[g.n] = b->mask;
      g.vals[g.n] = b->vals;
      g.seg_times[g.n] = b->seg_times;
      g.coeffs[g.n] = b->coeffs;
      g.status[g.n] = b->status;
      g.cost[g.n] = b->cost;
      g.pos_wp[g.n] = (b->opt.flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) ? b->wp : nullptr;
      waypoints = waypoints && g.pos_wp[g.n] != nullptr;
      // MRS_TG_FLAG_CONSTRAINED_SLOTS of any batch of the group: the dispatch runs the instantiations that take stop_at
      // vertices inside the specialised sweeps
      hints.constrained_slots = hints.constrained_slots || (b->opt.flags & MRS_TG_FLAG_CONSTRAINED_SLOTS) != 0;
    }
    if (plan->view.n_paths == 0) continue;
    HIP_TRY(ctx, use_device(ctx->device));
    ProfileScope ps(ctx, 1);
    const mrs_tg::SolveRoute route = group_route(plan->view, first->opt.derivative_to_optimize, hints, g.n, waypoints);
    if (mrs_tg::uses_factor_store(route)) {
      // the dispatch carries more paths than the rows kernel has wavefront slots for: four or eight lanes per path, factors in
      // LDS (one factor store per batch of THIS group; grows when a larger group comes, never shrinks)
      HIP_TRY(ctx, plan->d_ws.ensure((size_t)g.n * mrs_tg::linear_workspace_doubles(plan->view), mrs_tg::StreamIdle{ctx->stream}));
      HIP_TRY(ctx, mrs_tg::launch_solve_quad_group(plan->view, route, g, plan->d_ws.get(), ctx->stream));
    } else {
      HIP_TRY(ctx, mrs_tg::launch_solve_rows_group(plan->view, route, g, ctx->stream));
    }
  }
  return MRS_TG_OK;
}

// The routing table, from the routers themselves: the calling thread runs the very launch functions a solve would run, in dry
// mode -- every size rule, environment knob and hint takes effect, kernels are noted instead of enqueued.
int mrs_tg_plan_explain(mrs_tg_plan* plan, const mrs_tg_options* opt, int32_t group_size, const char** names_out, int32_t capacity) {
  if (!plan || !names_out || capacity <= 0) return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "plan, names_out and a positive capacity are required");
  mrs_tg_ctx* ctx = plan->ctx;
  int rc = check_options(ctx, opt);
  if (rc != MRS_TG_OK) return rc;
  if (group_size < 0 || group_size > mrs_tg::kRowsGroupMax)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "group_size %d: a dispatch carries 1 .. %d batches (0 = a single solve)", group_size, mrs_tg::kRowsGroupMax);
  // stand-ins for the caller's device arrays: never dereferenced (nothing is enqueued), only tested against NULL
  static double dummy_d[4];
  static uint8_t dummy_b[4];
  static int32_t dummy_i[4];
  struct DryScope {
    mrs_tg_ctx* c;
    bool was_profiling;
    explicit DryScope(mrs_tg_ctx* ctx_) : c(ctx_), was_profiling(ctx_->profiling) {
      c->profiling = false;  // (no events are armed for launches that do not happen)
      mrs_tg::set_dry_run(true);
      mrs_tg::kernel_trace_reset();
    }
    ~DryScope() {
      mrs_tg::set_dry_run(false);
      c->profiling = was_profiling;
    }
  };
  {
    DryScope scope(ctx);
    if (group_size == 0) {
      rc = mrs_tg_plan_solve(plan, dummy_d, dummy_b, dummy_d, dummy_d, opt, dummy_d, dummy_d, dummy_i, dummy_d,
                             opt->sampling_dt > 0 ? dummy_i : nullptr, opt->sampling_dt > 0 ? dummy_d : nullptr);
    } else {
      std::vector<mrs_tg_bound_solve> solves((size_t)group_size,
                                             mrs_tg_bound_solve{plan, dummy_d, dummy_b, dummy_d, dummy_d, *opt, dummy_d, dummy_d, dummy_i, dummy_d, nullptr, nullptr});
      std::vector<mrs_tg_bound_solve*> ptrs;
      for (mrs_tg_bound_solve& b : solves) ptrs.push_back(&b);
      rc = mrs_tg_bound_solve_launch_group(ptrs.data(), group_size, group_size);
    }
  }
  if (rc != MRS_TG_OK) return rc;
  return mrs_tg::kernel_trace(names_out, capacity);
}

int mrs_tg_plan_cost_gradient(mrs_tg_plan* plan, int32_t d, const uint8_t* mask, const double* vals,
                              const double* seg_times, double* cost, double* grad) {
  if (!plan || !mask || !vals || !seg_times || !cost || !grad)
    return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  if (d < 0 || d > 4) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize %d outside [0, 4]", d);
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, mrs_tg::launch_cost_gradient(plan->nl, plan->view, d, mask, vals, seg_times, cost, grad, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_segment_maxima(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, double* maxima) {
  if (!plan || !coeffs || !seg_times || !maxima)
    return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, mrs_tg::launch_segment_maxima(plan->view, coeffs, seg_times, maxima, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_segment_maxima_vjp(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, const double* grad_maxima,
                                   double* grad_coeffs, double* grad_times, double* argmax) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!coeffs || !seg_times || !grad_maxima)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "coeffs, seg_times and grad_maxima are required");
  if (!grad_coeffs && !grad_times && !argmax)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_coeffs_out, grad_seg_times_out and argmax_out are all NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 4);
  HIP_TRY(ctx, mrs_tg::launch_segment_maxima_vjp(plan->view.n_segments, coeffs, seg_times, grad_maxima, grad_coeffs, grad_times,
                                                 argmax, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_solve_vjp(mrs_tg_plan* plan, int32_t d, const uint8_t* mask, const double* vals, const double* seg_times,
                          const double* coeffs, const int32_t* status, const double* grad_coeffs, const double* grad_cost,
                          double* grad_vals, double* grad_times) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!mask || !vals || !seg_times || !coeffs || !status)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "fixed_mask, fixed_values, seg_times, coeffs and status are required");
  if (!grad_coeffs && !grad_cost) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_coeffs and grad_cost are both NULL");
  if (!grad_vals && !grad_times)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_fixed_values_out and grad_seg_times_out are both NULL");
  if (d < 0 || d > 4) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize %d outside [0, 4]", d);
  HIP_TRY(ctx, use_device(ctx->device));
  const mrs_tg::BatchView& b = plan->view;
  HIP_TRY(ctx, plan->d_ws.ensure(mrs_tg::vjp_workspace_doubles(b), mrs_tg::StreamIdle{ctx->stream}));
  ProfileScope ps(ctx, 3);
  HIP_TRY(ctx, mrs_tg::launch_vjp(b, d, mask, vals, seg_times, coeffs, status, grad_coeffs, grad_cost, plan->d_ws.get(), grad_vals,
                                  grad_times, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_careful_count(mrs_tg_plan* plan, int32_t* count_out) {
  if (!plan || !count_out) return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  *count_out = 0;
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (!plan->nl.d_careful.get()) return MRS_TG_OK;  // no outer loop has run on this plan
  HIP_TRY(ctx, hipMemcpy(count_out, plan->nl.d_careful.get() + 2, sizeof(int32_t), hipMemcpyDeviceToHost));
  return MRS_TG_OK;
}

int mrs_tg_plan_sample_states(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, double sampling_dt,
                              int32_t sample_capacity, int32_t* n_samples, double* states) {
  if (!plan || !coeffs || !seg_times || !n_samples)
    return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!(sampling_dt > 0.0) || sample_capacity < 0 || (sample_capacity > 0 && !states))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sampling_dt must be positive and states_out_dev given for a positive capacity");
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, mrs_tg::launch_sample_states(plan->view, coeffs, seg_times, sampling_dt, sample_capacity, n_samples,
                                            sample_capacity > 0 ? states : nullptr, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_sample(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, double sampling_dt,
                       int32_t sample_capacity, int32_t* n_samples, double* samples) {
  if (!plan || !coeffs || !seg_times || !n_samples)
    return fail(plan ? plan->ctx : nullptr, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!(sampling_dt > 0.0) || sample_capacity < 0 || (sample_capacity > 0 && !samples))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sampling_dt must be positive and samples_out_dev given for a positive capacity");
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, mrs_tg::launch_sample(plan->view, coeffs, seg_times, sampling_dt, sample_capacity, n_samples,
                                     sample_capacity > 0 ? samples : nullptr, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_sample_states_vjp(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, double sampling_dt,
                                  int32_t sample_capacity, int32_t n_orders, const double* grad_states, const int32_t* status,
                                  double* grad_coeffs, double* grad_times, int32_t* sample_segment, double* sample_time,
                                  int32_t* n_samples) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!coeffs || !seg_times) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "coeffs and seg_times are required");
  if (!(sampling_dt > 0.0) || sample_capacity < 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sampling_dt must be positive and sample_capacity non-negative");
  if (int rc = check_n_orders(ctx, n_orders)) return rc;
  if (!grad_coeffs && !grad_times && !sample_segment && !sample_time && !n_samples)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "grad_coeffs_out, grad_seg_times_out, sample_segment_out, sample_time_out and n_samples_out are all NULL");
  if ((grad_coeffs || grad_times) && !grad_states)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_coeffs_out and grad_seg_times_out need the upstream grad_states");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 5);
  HIP_TRY(ctx, mrs_tg::launch_sample_vjp(plan->view, coeffs, seg_times, sampling_dt, sample_capacity, n_orders, grad_states, status,
                                         grad_coeffs, grad_times, sample_segment, sample_time, n_samples, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_evaluate(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, const double* query_times,
                         int32_t n_queries, int32_t n_orders, double* states, int32_t* query_segment, double* query_local_time) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (n_queries < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_queries %d is negative", n_queries);
  if (int rc = check_n_orders(ctx, n_orders)) return rc;
  if (!coeffs || !seg_times) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "coeffs and seg_times are required");
  if (n_queries > 0 && (!query_times || !states))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "query_times_dev and states_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 6);
  return staged_launch_result(ctx, plan,
                              mrs_tg::launch_evaluate(plan->view, coeffs, seg_times, query_times, n_queries, n_orders, states,
                                                      query_segment, query_local_time, ctx->stream));
}

int mrs_tg_plan_evaluate_vjp(mrs_tg_plan* plan, const double* coeffs, const double* seg_times, const double* query_times,
                             int32_t n_queries, int32_t n_orders, const double* grad_states, const int32_t* status,
                             double* grad_coeffs, double* grad_times, double* grad_query_times) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (n_queries < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_queries %d is negative", n_queries);
  if (int rc = check_n_orders(ctx, n_orders)) return rc;
  if (!coeffs || !seg_times) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "coeffs and seg_times are required");
  if (n_queries > 0 && (!query_times || !grad_states))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "query_times_dev and grad_states_dev are required");
  if (!grad_coeffs && !grad_times && !grad_query_times)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_coeffs_out, grad_seg_times_out and grad_query_times_out are all NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 7);
  return staged_launch_result(ctx, plan,
                              mrs_tg::launch_evaluate_vjp(plan->view, coeffs, seg_times, query_times, n_queries, n_orders, grad_states,
                                                          status, grad_coeffs, grad_times, grad_query_times, ctx->stream));
}

// the sample rows of a plan step: a capacity, the counts, the rows where there are any
static int sample_rows_present(mrs_tg_ctx* ctx, const double* samples, const int32_t* n_samples, int32_t capacity) {
  if (capacity < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sample_capacity %d is negative", capacity);
  if (!n_samples) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_samples_dev is NULL");
  if (capacity > 0 && !samples) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "samples_dev is NULL with rows");
  return MRS_TG_OK;
}

int mrs_tg_plan_path_deviation(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                               const double* waypoints, int32_t first_segment, const int32_t* status, double* deviation,
                               int32_t* cursor, double* max_deviation, int32_t* argmax, double* segment_max) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!waypoints) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev is NULL");
  if (!deviation && !cursor && !max_deviation && !argmax && !segment_max)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_path_deviation is NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 8);
  return staged_launch_result(ctx, plan,
                              mrs_tg::launch_path_deviation(plan->view, samples, n_samples, waypoints, sample_capacity, first_segment,
                                                            status, deviation, cursor, max_deviation, argmax, segment_max,
                                                            ctx->stream));
}

int mrs_tg_plan_path_deviation_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                   const double* waypoints, const int32_t* status, const double* grad_deviation,
                                   double* grad_samples, double* grad_waypoints) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!waypoints || (sample_capacity > 0 && !grad_deviation))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev and grad_deviation_dev are required");
  if (!grad_samples && !grad_waypoints)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_samples_out and grad_waypoints_out are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 9);
  return staged_launch_result(ctx, plan,
                              mrs_tg::launch_path_deviation_vjp(plan->view, samples, n_samples, waypoints, sample_capacity, status,
                                                                grad_deviation, grad_samples, grad_waypoints, ctx->stream));
}

int mrs_tg_plan_estimate_times(mrs_tg_plan* plan, const double* waypoints, const double* limits, double* seg_times_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !limits || !seg_times_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev, limits_dev and seg_times_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 10);
  HIP_TRY(ctx, mrs_tg::launch_estimate_times(plan->view, waypoints, limits, seg_times_out, ctx->stream, /*timed=*/true));
  return MRS_TG_OK;
}

int mrs_tg_plan_estimate_times_vjp(mrs_tg_plan* plan, const double* waypoints, const double* limits,
                                   const double* grad_seg_times, double* grad_waypoints, double* grad_limits, int32_t* term) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !limits) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev and limits_dev are required");
  if (!grad_waypoints && !grad_limits && !term)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_estimate_times_vjp is NULL");
  if ((grad_waypoints || grad_limits) && !grad_seg_times)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_waypoints_out_dev and grad_limits_out_dev need grad_seg_times_dev");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 11);
  HIP_TRY(ctx, mrs_tg::launch_estimate_times_vjp(plan->view, waypoints, limits, grad_seg_times, grad_waypoints, grad_limits,
                                                 term, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_waypoint_passage(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                 const int32_t* wp_offsets, const double* waypoints, const int32_t* status, int32_t* index,
                                 int32_t* count, double* miss, double* fraction) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!waypoints) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev is NULL");
  if (!index && !count && !miss && !fraction)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_waypoint_passage is NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 12);
  HIP_TRY(ctx, mrs_tg::launch_waypoint_passage(plan->view, samples, n_samples, sample_capacity, wp_offsets, waypoints, status,
                                               index, count, miss, fraction, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_waypoint_passage_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                     const int32_t* wp_offsets, const double* waypoints, const int32_t* status,
                                     const double* grad_miss, const double* grad_fraction, double* grad_samples,
                                     double* grad_waypoints) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!waypoints) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev is NULL");
  if (!grad_samples && !grad_waypoints)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_samples_out and grad_waypoints_out are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 13);
  HIP_TRY(ctx, mrs_tg::launch_waypoint_passage_vjp(plan->view, samples, n_samples, sample_capacity, wp_offsets, waypoints, status,
                                                   grad_miss, grad_fraction, grad_samples, grad_waypoints, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_estimate_times_baca(mrs_tg_plan* plan, const double* waypoints, const double* limits, double* seg_times_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !limits || !seg_times_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev, limits_dev and seg_times_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 14);
  HIP_TRY(ctx, mrs_tg::launch_baca_times(plan->view, waypoints, limits, seg_times_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_estimate_times_baca_vjp(mrs_tg_plan* plan, const double* waypoints, const double* limits,
                                        const double* grad_seg_times, double* grad_waypoints, double* grad_limits,
                                        int32_t* flags) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !limits) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev and limits_dev are required");
  if (!grad_waypoints && !grad_limits && !flags)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_estimate_times_baca_vjp is NULL");
  if ((grad_waypoints || grad_limits) && !grad_seg_times)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_waypoints_out_dev and grad_limits_out_dev need grad_seg_times_dev");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 15);
  HIP_TRY(ctx, mrs_tg::launch_baca_times_vjp(plan->view, waypoints, limits, grad_seg_times, grad_waypoints, grad_limits, flags,
                                             ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_length_gate(mrs_tg_plan* plan, const double* seg_times, const int32_t* n_samples, double sampling_dt,
                            double max_factor, double min_factor, const int32_t* status, double* total_out, int32_t* verdict_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!seg_times || !n_samples) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "seg_times_dev and n_samples_dev are required");
  if (!total_out && !verdict_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "total_out_dev and verdict_out_dev are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 16);
  HIP_TRY(ctx, mrs_tg::launch_length_gate(plan->view, seg_times, n_samples, sampling_dt, max_factor, min_factor, status, total_out,
                                          verdict_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_unwrap_headings(mrs_tg_plan* plan, const double* waypoints, double* waypoints_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !waypoints_out) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev and waypoints_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 17);
  HIP_TRY(ctx, mrs_tg::launch_unwrap_headings(plan->view, waypoints, waypoints_out, ctx->stream));
  return MRS_TG_OK;
}

// what the two fallback calls check before any launch -> MRS_TG_OK and the dwell's row count
static int fallback_arguments(mrs_tg_ctx* ctx, double sampling_dt, double stopping_time, int32_t sample_capacity,
                              int32_t* insert) {
  if (!(sampling_dt > 0.0) || !std::isfinite(sampling_dt))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sampling_dt must be positive and finite");
  if (!(stopping_time >= 0.0) || !std::isfinite(stopping_time))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "stopping_time must be non-negative and finite");
  if (!mrs_tg::fbq::insert_count(stopping_time, sampling_dt, insert))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "round(stopping_time / sampling_dt) does not fit int32");
  if (sample_capacity < 1 || sample_capacity > mrs_tg::fbq::kMaxCapacity)  // (capacity + 1 is a value the outputs report)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sample_capacity must be in [1, %d]", mrs_tg::fbq::kMaxCapacity);
  return MRS_TG_OK;
}

int mrs_tg_plan_fallback_sample(mrs_tg_plan* plan, const double* waypoints, const uint8_t* stop_at, const double* seg_times,
                                double sampling_dt, double stopping_time, int32_t sample_capacity, int32_t* n_samples_out,
                                double* samples_out, int32_t* seg_first_row_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !seg_times || !n_samples_out || !samples_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev, seg_times_dev, n_samples_out_dev and samples_out_dev are required");
  int32_t insert = 0;
  if (const int rc = fallback_arguments(ctx, sampling_dt, stopping_time, sample_capacity, &insert); rc != MRS_TG_OK) return rc;
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 18);
  HIP_TRY(ctx, mrs_tg::launch_fallback_sample(plan->view, waypoints, stop_at, seg_times, sampling_dt, insert, sample_capacity,
                                              n_samples_out, samples_out, seg_first_row_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_fallback_sample_vjp(mrs_tg_plan* plan, const uint8_t* stop_at, const double* seg_times, double sampling_dt,
                                    double stopping_time, int32_t sample_capacity, const double* grad_samples,
                                    double* grad_waypoints_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!seg_times || !grad_samples || !grad_waypoints_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "seg_times_dev, grad_samples_dev and grad_waypoints_out_dev are required");
  int32_t insert = 0;
  if (const int rc = fallback_arguments(ctx, sampling_dt, stopping_time, sample_capacity, &insert); rc != MRS_TG_OK) return rc;
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 19);
  HIP_TRY(ctx, mrs_tg::launch_fallback_sample_vjp(plan->view, stop_at, seg_times, sampling_dt, insert, sample_capacity,
                                                  grad_samples, grad_waypoints_out, ctx->stream));
  return MRS_TG_OK;
}

// what the two path-edit steps check before any launch: the bound on the edited batch's vertices fits int32, the scratch is there
static int path_edit_ready(mrs_tg_plan* plan, long long upper_bound) {
  mrs_tg_ctx* ctx = plan->ctx;
  if (upper_bound > 2147483647ll)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "the edited batch may have %lld vertices, which does not fit int32", upper_bound);
  HIP_TRY(ctx, use_device(ctx->device));
  HIP_TRY(ctx, plan->d_edit_ws.ensure((size_t)plan->view.n_segments + (size_t)plan->view.n_paths));
  return MRS_TG_OK;
}

int mrs_tg_plan_preprocess_path(mrs_tg_plan* plan, const double* waypoints, const uint8_t* stop_at, double min_waypoint_distance,
                                int32_t straightener_enabled, double straightener_max_deviation,
                                double straightener_max_hdg_deviation, int32_t* vertex_offsets_out, double* waypoints_out,
                                uint8_t* stop_at_out, int32_t* source_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !vertex_offsets_out || !waypoints_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev, vertex_offsets_out_dev and waypoints_out_dev are required");
  if (!(min_waypoint_distance >= 0.0) || !(straightener_max_deviation >= 0.0) || !(straightener_max_hdg_deviation >= 0.0))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "min_waypoint_distance and the straightener's thresholds must be non-negative numbers");
  if (const int rc = path_edit_ready(plan, (long long)plan->view.n_segments + plan->view.n_paths); rc != MRS_TG_OK) return rc;
  const mrs_tg::pathq::ThinOptions o{min_waypoint_distance, straightener_enabled != 0, straightener_max_deviation,
                                     straightener_max_hdg_deviation};
  ProfileScope ps(ctx, 20);
  HIP_TRY(ctx, mrs_tg::launch_preprocess_path(plan->view, waypoints, stop_at, o, plan->d_edit_ws.get(), vertex_offsets_out,
                                              waypoints_out, stop_at_out, source_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_insert_midpoints(mrs_tg_plan* plan, const double* waypoints, const uint8_t* stop_at, const double* segment_max,
                                 double max_deviation, int32_t first_segment, const uint8_t* active, int32_t* vertex_offsets_out,
                                 double* waypoints_out, uint8_t* stop_at_out, int32_t* source_out, uint8_t* inserted_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints || !segment_max || !vertex_offsets_out || !waypoints_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "waypoints_dev, segment_max_dev, vertex_offsets_out_dev and waypoints_out_dev are required");
  if (!(max_deviation >= 0.0)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "max_deviation must be a non-negative number");
  if (const int rc = path_edit_ready(plan, 2ll * plan->view.n_segments + plan->view.n_paths); rc != MRS_TG_OK) return rc;
  ProfileScope ps(ctx, 21);
  HIP_TRY(ctx, mrs_tg::launch_insert_midpoints(plan->view, waypoints, stop_at, segment_max, max_deviation, first_segment != 0, active,
                                               plan->d_edit_ws.get(), vertex_offsets_out, waypoints_out, stop_at_out, source_out,
                                               inserted_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_path_edit_vjp(mrs_tg_plan* plan, const int32_t* vertex_offsets, const int32_t* source, const uint8_t* inserted,
                              const double* grad_waypoints_edited, double* grad_waypoints_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!vertex_offsets || !source || !grad_waypoints_edited || !grad_waypoints_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "vertex_offsets_dev, source_dev, grad_waypoints_edited_dev and grad_waypoints_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 22);
  HIP_TRY(ctx, mrs_tg::launch_path_edit_vjp(plan->view, vertex_offsets, source, inserted, grad_waypoints_edited, grad_waypoints_out,
                                            ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_travel_heading(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                               const int32_t* status, double min_step, double* samples_out, int32_t* source_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!std::isfinite(min_step)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "min_step must be finite");
  if (sample_capacity > 0 && !samples_out) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "samples_out_dev is required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 23);
  HIP_TRY(ctx, mrs_tg::launch_travel_heading(plan->view.n_paths, samples, n_samples, sample_capacity, status, min_step, samples_out,
                                             source_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_travel_heading_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                   const int32_t* status, double min_step, const double* grad_out, double* grad_samples) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = sample_rows_present(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!std::isfinite(min_step)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "min_step must be finite");
  if (sample_capacity > 0 && (!grad_out || !grad_samples))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_out_dev and grad_samples_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 24);
  HIP_TRY(ctx, mrs_tg::launch_travel_heading_vjp(plan->view.n_paths, samples, n_samples, sample_capacity, status, min_step, grad_out,
                                                 grad_samples, ctx->stream));
  return MRS_TG_OK;
}

// ---- initial condition, prepend and prediction splice as plan steps (mrs_tg_initial.hip) ------------------------------------

// what the six calls check of their sizes before any launch: no negative capacity, no sum beyond int32
static int initial_sizes(mrs_tg_ctx* ctx, const mrs_tg_plan* plan, long long n_vertices, long long sample_capacity,
                         long long pred_capacity) {
  if (n_vertices < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_vertices %lld is negative", n_vertices);
  if (sample_capacity < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sample_capacity %lld is negative", sample_capacity);
  if (pred_capacity < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "pred_capacity %lld is negative", pred_capacity);
  if (n_vertices + plan->view.n_paths > 2147483647ll)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "%lld requested vertices and %d prepended ones do not fit int32", n_vertices,
                plan->view.n_paths);
  if (sample_capacity + pred_capacity > 2147483647ll)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "sample_capacity %lld + pred_capacity %lld does not fit int32", sample_capacity,
                pred_capacity);
  return MRS_TG_OK;
}

int mrs_tg_plan_initial_condition(mrs_tg_plan* plan, const int32_t* flags, const double* tracker, const double* tracker_age,
                                  const double* uav_pose, double takeoff_height, const double* path_time_offset,
                                  const int32_t* vertex_offsets, const double* pred_position, const double* pred_velocity,
                                  const double* pred_acceleration, const double* pred_jerk, const int32_t* n_pred,
                                  int32_t pred_capacity, int32_t* decision_out, int32_t* sample_offset_out, double* initial_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = initial_sizes(ctx, plan, 0, 0, pred_capacity); rc != MRS_TG_OK) return rc;
  if (!flags || !tracker || !tracker_age || !uav_pose || !path_time_offset || !vertex_offsets || !n_pred)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "flags_dev, tracker_dev, tracker_age_dev, uav_pose_dev, path_time_offset_dev, vertex_offsets_dev and n_pred_dev "
                "are required");
  if (pred_capacity > 0 && (!pred_position || !pred_velocity || !pred_acceleration || !pred_jerk))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "a prediction with rows needs all four arrays");
  if (!decision_out || !sample_offset_out || !initial_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "decision_out_dev, sample_offset_out_dev and initial_out_dev are required");
  if (std::isnan(takeoff_height)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "takeoff_height is NaN");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 25);
  const double* const pred[4] = {pred_position, pred_velocity, pred_acceleration, pred_jerk};
  HIP_TRY(ctx, mrs_tg::launch_initial_condition(plan->view.n_paths, flags, tracker, tracker_age, uav_pose, takeoff_height,
                                                path_time_offset, vertex_offsets, pred, n_pred, pred_capacity, decision_out,
                                                sample_offset_out, initial_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_initial_condition_vjp(mrs_tg_plan* plan, const int32_t* decision, const int32_t* sample_offset,
                                      const double* grad_initial, int32_t pred_capacity, double* grad_tracker_out,
                                      double* grad_uav_out, double* grad_pred_position_out, double* grad_pred_velocity_out,
                                      double* grad_pred_acceleration_out, double* grad_pred_jerk_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = initial_sizes(ctx, plan, 0, 0, pred_capacity); rc != MRS_TG_OK) return rc;
  if (!decision || !sample_offset || !grad_initial || !grad_tracker_out || !grad_uav_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "decision_dev, sample_offset_dev, grad_initial_dev, grad_tracker_out_dev and grad_uav_out_dev are required");
  if (pred_capacity > 0 && (!grad_pred_position_out || !grad_pred_velocity_out || !grad_pred_acceleration_out || !grad_pred_jerk_out))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "a prediction with rows needs all four gradient arrays");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 29);
  double* const grad_pred[4] = {grad_pred_position_out, grad_pred_velocity_out, grad_pred_acceleration_out, grad_pred_jerk_out};
  HIP_TRY(ctx, mrs_tg::launch_initial_condition_vjp(plan->view.n_paths, decision, sample_offset, grad_initial, pred_capacity,
                                                    grad_tracker_out, grad_uav_out, grad_pred, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_prepend_initial_condition(mrs_tg_plan* plan, const int32_t* vertex_offsets, int32_t n_vertices,
                                          const double* waypoints, const uint8_t* stop_at, const int32_t* decision,
                                          const double* initial, int32_t* vertex_offsets_out, double* waypoints_out,
                                          uint8_t* stop_at_out, int32_t* source_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = initial_sizes(ctx, plan, n_vertices, 0, 0); rc != MRS_TG_OK) return rc;
  if (!vertex_offsets || !decision || !initial || !vertex_offsets_out || !waypoints_out || (n_vertices > 0 && !waypoints))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "vertex_offsets_dev, waypoints_dev, decision_dev, initial_dev, vertex_offsets_out_dev and waypoints_out_dev are "
                "required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 26);
  HIP_TRY(ctx, mrs_tg::launch_prepend_initial_condition(plan->view.n_paths, n_vertices, vertex_offsets, waypoints, stop_at, decision,
                                                        initial, vertex_offsets_out, waypoints_out, stop_at_out, source_out,
                                                        ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_prepend_initial_condition_vjp(mrs_tg_plan* plan, const int32_t* vertex_offsets, int32_t n_vertices,
                                              const int32_t* decision, const int32_t* vertex_offsets_edited, int32_t n_vertices_edited,
                                              const double* grad_waypoints_edited, double* grad_waypoints_out,
                                              double* grad_initial_row_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = initial_sizes(ctx, plan, n_vertices, 0, 0); rc != MRS_TG_OK) return rc;
  if (n_vertices_edited < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_vertices_edited %d is negative", n_vertices_edited);
  if (!vertex_offsets || !decision || !vertex_offsets_edited || !grad_initial_row_out || (n_vertices > 0 && !grad_waypoints_out) ||
      (n_vertices_edited > 0 && !grad_waypoints_edited))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "vertex_offsets_dev, decision_dev, vertex_offsets_edited_dev, grad_waypoints_edited_dev, grad_waypoints_out_dev and "
                "grad_initial_row_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 30);
  HIP_TRY(ctx, mrs_tg::launch_prepend_initial_condition_vjp(plan->view.n_paths, n_vertices, vertex_offsets, decision,
                                                            vertex_offsets_edited, n_vertices_edited, grad_waypoints_edited,
                                                            grad_waypoints_out, grad_initial_row_out, ctx->stream));
  return MRS_TG_OK;
}

// what the splice and its backward pass check of the arrays they share
static int splice_arguments(mrs_tg_ctx* ctx, const mrs_tg_plan* plan, const int32_t* n_samples, int32_t sample_capacity,
                            const int32_t* decision, const int32_t* sample_offset, const double* prediction_age,
                            const int32_t* n_pred, int32_t pred_capacity) {
  if (const int rc = initial_sizes(ctx, plan, 0, sample_capacity, pred_capacity); rc != MRS_TG_OK) return rc;
  if (!n_samples || !decision || !sample_offset || !prediction_age || !n_pred)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                "n_samples_dev, decision_dev, sample_offset_dev, prediction_age_dev and n_pred_dev are required");
  return MRS_TG_OK;
}

int mrs_tg_plan_splice_prediction(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                  const int32_t* status, const int32_t* decision, const int32_t* sample_offset,
                                  const double* prediction_age, const double* pred_position, const int32_t* n_pred,
                                  int32_t pred_capacity, double* samples_out, int32_t* n_samples_out, int32_t* status_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = splice_arguments(ctx, plan, n_samples, sample_capacity, decision, sample_offset, prediction_age, n_pred,
                                      pred_capacity);
      rc != MRS_TG_OK)
    return rc;
  if (!n_samples_out || (sample_capacity > 0 && (!samples || !samples_out)) || (pred_capacity > 0 && !pred_position))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "samples_dev, pred_position_dev, samples_out_dev and n_samples_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 27);
  HIP_TRY(ctx, mrs_tg::launch_splice_prediction(plan->view.n_paths, samples, n_samples, sample_capacity, status, decision,
                                                sample_offset, prediction_age, pred_position, n_pred, pred_capacity, samples_out,
                                                n_samples_out, status_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_splice_prediction_vjp(mrs_tg_plan* plan, const int32_t* n_samples, int32_t sample_capacity, const int32_t* status,
                                      const int32_t* decision, const int32_t* sample_offset, const double* prediction_age,
                                      const int32_t* n_pred, int32_t pred_capacity, const double* grad_out, double* grad_samples_out,
                                      double* grad_pred_position_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = splice_arguments(ctx, plan, n_samples, sample_capacity, decision, sample_offset, prediction_age, n_pred,
                                      pred_capacity);
      rc != MRS_TG_OK)
    return rc;
  if ((sample_capacity > 0 && (!grad_out || !grad_samples_out)) || (pred_capacity > 0 && !grad_pred_position_out))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_out_dev, grad_samples_out_dev and grad_pred_position_out_dev are required");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 28);
  HIP_TRY(ctx, mrs_tg::launch_splice_prediction_vjp(plan->view.n_paths, n_samples, sample_capacity, status, decision, sample_offset,
                                                    prediction_age, n_pred, pred_capacity, grad_out, grad_samples_out,
                                                    grad_pred_position_out, ctx->stream));
  return MRS_TG_OK;
}

// ---- the request's vertices and limits as plan steps (mrs_tg_request.hip) -------------------------------------------------------

int mrs_tg_plan_request_vertices(mrs_tg_plan* plan, const double* waypoints, const uint8_t* stop_at, const uint8_t* has_state,
                                 const double* state, int32_t derivative_to_optimize, double* waypoints_out, uint8_t* fixed_mask_out,
                                 double* fixed_values_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!waypoints) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_dev is required");
  if (derivative_to_optimize < 2 || derivative_to_optimize > 4)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize must be 2, 3 or 4 (got %d)", derivative_to_optimize);
  if (has_state && !state) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "has_state_dev without state_dev");
  if (!waypoints_out && !fixed_mask_out && !fixed_values_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "waypoints_out_dev, fixed_mask_out_dev and fixed_values_out_dev are all NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 31);
  HIP_TRY(ctx, mrs_tg::launch_request_vertices(plan->view, waypoints, stop_at, has_state, state, derivative_to_optimize,
                                               waypoints_out, fixed_mask_out, fixed_values_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_request_vertices_vjp(mrs_tg_plan* plan, const uint8_t* has_state, const double* grad_waypoints,
                                     const double* grad_fixed_values, double* grad_waypoints_out, double* grad_state_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!grad_waypoints && !grad_fixed_values)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_waypoints_dev and grad_fixed_values_dev are both NULL: no upstream");
  if (!grad_waypoints_out && !grad_state_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_waypoints_out_dev and grad_state_out_dev are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 32);
  HIP_TRY(ctx, mrs_tg::launch_request_vertices_vjp(plan->view, has_state, grad_waypoints, grad_fixed_values, grad_waypoints_out,
                                                   grad_state_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_request_limits(mrs_tg_plan* plan, const double* constraints, const double* override_, const int32_t* flags,
                               const uint8_t* has_state, const double* state, int32_t fallback, double speed_factor,
                               double accel_factor, double* limits_out, int32_t* branch_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!constraints) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "constraints_dev is required");
  if (flags && !override_) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "flags_dev without override_dev");
  if (has_state && !state) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "has_state_dev without state_dev");
  if (!limits_out && !branch_out) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "limits_out_dev and branch_out_dev are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 33);
  HIP_TRY(ctx, mrs_tg::launch_request_limits(plan->view.n_paths, constraints, override_, flags, has_state, state, fallback != 0,
                                             speed_factor, accel_factor, limits_out, branch_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_request_limits_vjp(mrs_tg_plan* plan, const int32_t* branch, int32_t fallback, double speed_factor,
                                   double accel_factor, const double* grad_limits, double* grad_constraints_out,
                                   double* grad_override_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (!branch) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "branch_dev is required");
  if (!grad_limits) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_limits_dev is NULL: no upstream");
  if (!grad_constraints_out && !grad_override_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_constraints_out_dev and grad_override_out_dev are both NULL");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 34);
  HIP_TRY(ctx, mrs_tg::launch_request_limits_vjp(plan->view.n_paths, branch, fallback != 0, speed_factor, accel_factor, grad_limits,
                                                 grad_constraints_out, grad_override_out, ctx->stream));
  return MRS_TG_OK;
}

// ---- the clearance steps: mutual (mrs_tg_clearance.hip), from obstacles (mrs_tg_obstacle.hip), from a field (mrs_tg_field.hip) ----

// ... and their alignment, which the clearance steps ask for (the older steps never did, and do not start now)
static int sample_rows_arguments(mrs_tg_ctx* ctx, const double* samples, const int32_t* n_samples, int32_t capacity) {
  if (const int rc = sample_rows_present(ctx, samples, n_samples, capacity); rc != MRS_TG_OK) return rc;
  if (((uintptr_t)samples & 15u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "samples_dev is not 16-byte aligned");
  if (((uintptr_t)n_samples & 3u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_samples_dev is not 4-byte aligned");
  return MRS_TG_OK;
}

// the backward passes' operands: the forward's tag array (named in the messages), the upstream and the output
static int backward_operands(mrs_tg_ctx* ctx, bool required, const int32_t* tag, const char* tag_name, const double* grad_clearance,
                             const double* grad_samples_out) {
  if (required && (!tag || !grad_clearance || !grad_samples_out))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "%s, grad_clearance_dev and grad_samples_out_dev are required", tag_name);
  if (((uintptr_t)grad_samples_out & 15u) == 0 && ((uintptr_t)grad_clearance & 7u) == 0 && ((uintptr_t)tag & 3u) == 0) return MRS_TG_OK;
  return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_samples_out_dev (16 bytes), grad_clearance_dev or %s is not aligned", tag_name);
}

// what the two mutual clearance calls check before any launch
static int mutual_clearance_arguments(mrs_tg_ctx* ctx, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                      const int32_t* group_offsets, int32_t n_groups, const int32_t* first_step,
                                      const int32_t* status, double z_scale) {
  if (const int rc = sample_rows_arguments(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (n_groups < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_groups %d is negative", n_groups);
  if (!group_offsets) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "group_offsets_dev is NULL");
  if (!(std::isfinite(z_scale) && z_scale > 0.0)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "z_scale must be finite and positive");
  if ((((uintptr_t)group_offsets | (uintptr_t)first_step | (uintptr_t)status) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an int32 array is not 4-byte aligned");
  return MRS_TG_OK;
}

int mrs_tg_plan_mutual_clearance(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                 const int32_t* group_offsets, int32_t n_groups, const int32_t* first_step, const int32_t* status,
                                 double z_scale, double* clearance_out, int32_t* partner_out, double* min_clearance_out,
                                 int32_t* argmin_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = mutual_clearance_arguments(ctx, samples, n_samples, sample_capacity, group_offsets, n_groups, first_step,
                                                status, z_scale);
      rc != MRS_TG_OK)
    return rc;
  // (at capacity 0 this step alone takes a forward without outputs and a backward without operands; the other two refuse both)
  if (sample_capacity > 0 && !clearance_out && !partner_out && !min_clearance_out && !argmin_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_mutual_clearance is NULL");
  if ((((uintptr_t)clearance_out | (uintptr_t)min_clearance_out) & 7u) != 0 ||
      (((uintptr_t)partner_out | (uintptr_t)argmin_out) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an output array is not aligned to its element");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 35);
  HIP_TRY(ctx, mrs_tg::launch_mutual_clearance(plan->view.n_paths, samples, n_samples, sample_capacity, group_offsets, n_groups,
                                               first_step, status, z_scale, clearance_out, partner_out, min_clearance_out,
                                               argmin_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_mutual_clearance_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                     const int32_t* group_offsets, int32_t n_groups, const int32_t* first_step,
                                     const int32_t* status, double z_scale, const int32_t* partner, const double* grad_clearance,
                                     double* grad_samples_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = mutual_clearance_arguments(ctx, samples, n_samples, sample_capacity, group_offsets, n_groups, first_step,
                                                status, z_scale);
      rc != MRS_TG_OK)
    return rc;
  if (const int rc = backward_operands(ctx, sample_capacity > 0, partner, "partner_dev", grad_clearance, grad_samples_out);
      rc != MRS_TG_OK)
    return rc;
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 36);
  HIP_TRY(ctx, mrs_tg::launch_mutual_clearance_vjp(plan->view.n_paths, samples, n_samples, sample_capacity, group_offsets, n_groups,
                                                   first_step, status, z_scale, partner, grad_clearance, grad_samples_out,
                                                   ctx->stream));
  return MRS_TG_OK;
}

// what the two obstacle calls check before any launch
static int obstacle_clearance_arguments(mrs_tg_ctx* ctx, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                        const double* obstacles, int32_t n_obstacles, const int32_t* set_offsets, int32_t n_sets,
                                        const int32_t* path_set, const int32_t* status, double z_scale) {
  if (const int rc = sample_rows_arguments(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (n_obstacles < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_obstacles %d is negative", n_obstacles);
  if (n_sets < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_sets %d is negative", n_sets);
  if (!set_offsets) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "set_offsets_dev is NULL");
  if (n_obstacles > 0 && !obstacles) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "obstacles_dev is NULL with %d obstacles", n_obstacles);
  if (!(std::isfinite(z_scale) && z_scale > 0.0)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "z_scale must be finite and positive");
  if (((uintptr_t)obstacles & 15u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "obstacles_dev is not 16-byte aligned");
  if ((((uintptr_t)set_offsets | (uintptr_t)path_set | (uintptr_t)status) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an int32 array is not 4-byte aligned");
  return MRS_TG_OK;
}

int mrs_tg_plan_obstacle_clearance(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                   const double* obstacles, int32_t n_obstacles, const int32_t* set_offsets, int32_t n_sets,
                                   const int32_t* path_set, const int32_t* status, double z_scale, double* clearance_out,
                                   int32_t* nearest_out, double* min_clearance_out, int32_t* argmin_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = obstacle_clearance_arguments(ctx, samples, n_samples, sample_capacity, obstacles, n_obstacles, set_offsets,
                                                  n_sets, path_set, status, z_scale);
      rc != MRS_TG_OK)
    return rc;
  if (!clearance_out && !nearest_out && !min_clearance_out && !argmin_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_obstacle_clearance is NULL");
  if ((((uintptr_t)clearance_out | (uintptr_t)min_clearance_out) & 7u) != 0 ||
      (((uintptr_t)nearest_out | (uintptr_t)argmin_out) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an output array is not aligned to its element");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 37);
  HIP_TRY(ctx, mrs_tg::launch_obstacle_clearance(plan->view.n_paths, samples, n_samples, sample_capacity, obstacles, n_obstacles,
                                                 set_offsets, n_sets, path_set, status, z_scale, clearance_out, nearest_out,
                                                 min_clearance_out, argmin_out, ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_obstacle_clearance_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                       const double* obstacles, int32_t n_obstacles, const int32_t* set_offsets, int32_t n_sets,
                                       const int32_t* path_set, const int32_t* status, double z_scale, const int32_t* nearest,
                                       const double* grad_clearance, double* grad_samples_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  if (const int rc = obstacle_clearance_arguments(ctx, samples, n_samples, sample_capacity, obstacles, n_obstacles, set_offsets,
                                                  n_sets, path_set, status, z_scale);
      rc != MRS_TG_OK)
    return rc;
  if (const int rc = backward_operands(ctx, true, nearest, "nearest_dev", grad_clearance, grad_samples_out); rc != MRS_TG_OK)
    return rc;
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 38);
  HIP_TRY(ctx, mrs_tg::launch_obstacle_clearance_vjp(plan->view.n_paths, samples, n_samples, sample_capacity, obstacles,
                                                     n_obstacles, set_offsets, n_sets, path_set, status, z_scale, nearest,
                                                     grad_clearance, grad_samples_out, ctx->stream));
  return MRS_TG_OK;
}

// what every call that takes a mrs_tg_field_geometry (not NULL) refuses in it; the number of voxels of the whole array
static int field_geometry_voxels(mrs_tg_ctx* ctx, const mrs_tg_field_geometry* geometry, long long* voxels_out) {
  if (geometry->n_fields < 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_fields %d is negative", geometry->n_fields);
  long long voxels = geometry->n_fields;
  for (int a = 0; a < 3; ++a) {
    if (geometry->dims[a] < 2) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "dims[%d] = %d is below 2", a, geometry->dims[a]);
    if (!(std::isfinite(geometry->spacing[a]) && geometry->spacing[a] > 0.0))
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "spacing[%d] must be finite and positive", a);
    if (!std::isfinite(geometry->origin[a])) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "origin[%d] is not finite", a);
    // (every factor is below 2^31 and the running product is held to 2^31 - 1: no overflow of the 64-bit product)
    voxels *= geometry->dims[a];
    if (voxels > 2147483647LL)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_fields nz ny nx exceeds 2^31 - 1: a cell is an int32");
  }
  *voxels_out = voxels;
  return MRS_TG_OK;
}

// what the two field calls check before any launch; fills the kernels' geometry
static int field_clearance_arguments(mrs_tg_ctx* ctx, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                     const double* fields, const mrs_tg_field_geometry* geometry, const int32_t* path_field,
                                     const int32_t* status, mrs_tg::fldq::Geometry* out) {
  if (const int rc = sample_rows_arguments(ctx, samples, n_samples, sample_capacity); rc != MRS_TG_OK) return rc;
  if (!geometry) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "geometry is NULL");
  long long voxels = 0;
  if (const int rc = field_geometry_voxels(ctx, geometry, &voxels); rc != MRS_TG_OK) return rc;
  if (geometry->n_fields > 0 && !fields) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "fields_dev is NULL with %d fields", geometry->n_fields);
  if ((((uintptr_t)fields) & 7u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "fields_dev is not 8-byte aligned");
  for (int a = 0; a < 3; ++a) out->o[a] = geometry->origin[a], out->h[a] = geometry->spacing[a], out->n[a] = geometry->dims[a];
  out->n_fields = geometry->n_fields;
  if ((((uintptr_t)path_field | (uintptr_t)status) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an int32 array is not 4-byte aligned");
  return MRS_TG_OK;
}

int mrs_tg_plan_field_clearance(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                const double* fields, const mrs_tg_field_geometry* geometry, const int32_t* path_field,
                                const int32_t* status, double outside_value, double* clearance_out, int32_t* cell_out,
                                double* gradient_out, double* min_clearance_out, int32_t* argmin_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  mrs_tg::fldq::Geometry G;
  if (const int rc = field_clearance_arguments(ctx, samples, n_samples, sample_capacity, fields, geometry, path_field, status, &G);
      rc != MRS_TG_OK)
    return rc;
  if (!clearance_out && !cell_out && !gradient_out && !min_clearance_out && !argmin_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "every output of mrs_tg_plan_field_clearance is NULL");
  if (((uintptr_t)gradient_out & 15u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "gradient_out_dev is not 16-byte aligned");
  if ((((uintptr_t)clearance_out | (uintptr_t)min_clearance_out) & 7u) != 0 ||
      (((uintptr_t)cell_out | (uintptr_t)argmin_out) & 3u) != 0)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "an output array is not aligned to its element");
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 39);
  HIP_TRY(ctx, mrs_tg::launch_field_clearance(plan->view.n_paths, samples, n_samples, sample_capacity, fields, G, path_field, status,
                                              outside_value, clearance_out, cell_out, gradient_out, min_clearance_out, argmin_out,
                                              ctx->stream));
  return MRS_TG_OK;
}

int mrs_tg_plan_field_clearance_vjp(mrs_tg_plan* plan, const double* samples, const int32_t* n_samples, int32_t sample_capacity,
                                    const double* fields, const mrs_tg_field_geometry* geometry, const int32_t* path_field,
                                    const int32_t* status, const int32_t* cell, const double* grad_clearance,
                                    double* grad_samples_out) {
  if (!plan) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "plan is NULL");
  mrs_tg_ctx* ctx = plan->ctx;
  mrs_tg::fldq::Geometry G;
  if (const int rc = field_clearance_arguments(ctx, samples, n_samples, sample_capacity, fields, geometry, path_field, status, &G);
      rc != MRS_TG_OK)
    return rc;
  if (const int rc = backward_operands(ctx, true, cell, "cell_dev", grad_clearance, grad_samples_out); rc != MRS_TG_OK) return rc;
  // the output may not overlap an input: the byte ranges the kernel touches
  const size_t P = (size_t)plan->view.n_paths, rows = P * (size_t)sample_capacity;
  const size_t voxels = (size_t)G.n_fields * (size_t)G.n[2] * (size_t)G.n[1] * (size_t)G.n[0];
  const uintptr_t out_lo = (uintptr_t)grad_samples_out, out_hi = out_lo + rows * 4 * sizeof(double);
  const struct {
    const void* at;
    size_t bytes;
    const char* name;
  } inputs[] = {{samples, rows * 4 * sizeof(double), "samples_dev"},       {n_samples, P * sizeof(int32_t), "n_samples_dev"},
                {fields, voxels * sizeof(double), "fields_dev"},            {path_field, P * sizeof(int32_t), "path_field_dev"},
                {status, P * sizeof(int32_t), "status_dev"},                {cell, rows * sizeof(int32_t), "cell_dev"},
                {grad_clearance, rows * sizeof(double), "grad_clearance_dev"}};
  for (const auto& in : inputs)
    if (in.at && in.bytes && (uintptr_t)in.at < out_hi && out_lo < (uintptr_t)in.at + in.bytes)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "grad_samples_out_dev overlaps %s", in.name);
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 40);
  HIP_TRY(ctx, mrs_tg::launch_field_clearance_vjp(plan->view.n_paths, samples, n_samples, sample_capacity, fields, G, path_field,
                                                  status, cell, grad_clearance, grad_samples_out, ctx->stream));
  return MRS_TG_OK;
}

// ---- the distance field from an occupancy grid (mrs_tg_edt.hip) -----------------------------------------------------------------------

// what mrs_tg_field_from_occupancy and mrs_tg_field_update_region refuse in the geometry and the scalars (geometry not NULL);
// ctx may be NULL (mrs_tg_field_update_query).  The number of voxels of the whole stack
static int occupancy_scalars(mrs_tg_ctx* ctx, const mrs_tg_field_geometry* geometry, double z_scale, double max_distance,
                             long long* voxels_out) {
  static_assert(MRS_TG_FIELD_SIGNED == mrs_tg::edtq::kSigned && MRS_TG_FIELD_MAX_DIM == mrs_tg::edtq::kMaxDim, "the header's");
  if (const int rc = field_geometry_voxels(ctx, geometry, voxels_out); rc != MRS_TG_OK) return rc;
  for (int a = 0; a < 3; ++a)
    if (geometry->dims[a] > MRS_TG_FIELD_MAX_DIM)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "dims[%d] = %d exceeds MRS_TG_FIELD_MAX_DIM = %d (a line is staged in LDS)", a,
                  geometry->dims[a], MRS_TG_FIELD_MAX_DIM);
  if (!(std::isfinite(z_scale) && z_scale > 0.0)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "z_scale must be finite and positive");
  if (!(max_distance > 0.0)) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "max_distance must be positive (+inf: no cap)");
  return MRS_TG_OK;
}

// ... and in the flags and the two arrays of the stack; `fields_name` is the header's name of the array of doubles
static int occupancy_arrays(mrs_tg_ctx* ctx, long long voxels, int32_t flags, const uint8_t* occupancy, const double* fields,
                            const char* fields_name) {
  if ((flags & ~MRS_TG_FIELD_SIGNED) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "unknown flag bits 0x%x", (unsigned)flags);
  if (voxels > 0 && (!occupancy || !fields))
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "occupancy_dev and %s are required with %lld voxels", fields_name, voxels);
  if (((uintptr_t)fields & 7u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "%s is not 8-byte aligned", fields_name);
  const uintptr_t out_lo = (uintptr_t)fields, out_hi = out_lo + (size_t)voxels * sizeof(double);
  if (voxels > 0 && (uintptr_t)occupancy < out_hi && out_lo < (uintptr_t)occupancy + (size_t)voxels)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "%s overlaps occupancy_dev", fields_name);
  return MRS_TG_OK;
}

int mrs_tg_field_from_occupancy(mrs_tg_ctx* ctx, const uint8_t* occupancy, const mrs_tg_field_geometry* geometry, double z_scale,
                                double max_distance, int32_t flags, double* fields_out) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  if (!geometry) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "geometry is NULL");
  long long voxels = 0;
  if (const int rc = occupancy_scalars(ctx, geometry, z_scale, max_distance, &voxels); rc != MRS_TG_OK) return rc;
  if (const int rc = occupancy_arrays(ctx, voxels, flags, occupancy, fields_out, "fields_out_dev"); rc != MRS_TG_OK) return rc;
  if (voxels == 0) return MRS_TG_OK;
  const bool is_signed = (flags & MRS_TG_FIELD_SIGNED) != 0;
  const double h[3] = {geometry->spacing[0], geometry->spacing[1], geometry->spacing[2]};
  const int dims[3] = {geometry->dims[0], geometry->dims[1], geometry->dims[2]};
  const mrs_tg::edtq::Weights W = mrs_tg::edtq::weights(h, z_scale);
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 41);
  HIP_TRY(ctx, mrs_tg::launch_field_from_occupancy(occupancy, dims, geometry->n_fields, W, mrs_tg::edtq::saturation(max_distance),
                                                   max_distance, is_signed, fields_out, ctx->stream));
  return MRS_TG_OK;
}

// ---- the distance field brought up to date after a change inside a box (mrs_tg_edt_region.hip) ------------------------------------------

// the plan of a region of a checked geometry (occupancy_scalars), or what is wrong with the region
static int field_region_plan(mrs_tg_ctx* ctx, const mrs_tg_field_geometry* geometry, double z_scale, double max_distance,
                             const mrs_tg_field_region* region, mrs_tg::edtq::RegionPlan* plan_out) {
  if (geometry->n_fields == 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_fields is 0: there is no grid to update");
  if (!region) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "region is NULL");
  if (region->field < 0 || region->field >= geometry->n_fields)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "region.field = %d is outside [0, %d)", region->field, geometry->n_fields);
  for (int a = 0; a < 3; ++a)
    if (region->lo[a] < 0 || region->hi[a] >= geometry->dims[a] || region->lo[a] > region->hi[a])
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "region axis %d: [%d, %d] is empty or not inside [0, %d]", a, region->lo[a],
                  region->hi[a], geometry->dims[a] - 1);
  const double h[3] = {geometry->spacing[0], geometry->spacing[1], geometry->spacing[2]};
  const int dims[3] = {geometry->dims[0], geometry->dims[1], geometry->dims[2]};
  const int lo[3] = {region->lo[0], region->lo[1], region->lo[2]}, hi[3] = {region->hi[0], region->hi[1], region->hi[2]};
  *plan_out = mrs_tg::edtq::plan_region(dims, mrs_tg::edtq::weights(h, z_scale), mrs_tg::edtq::saturation(max_distance), lo, hi);
  return MRS_TG_OK;
}

int mrs_tg_field_update_query(const mrs_tg_field_geometry* geometry, double z_scale, double max_distance,
                              const mrs_tg_field_region* region, mrs_tg_field_update_info* out) {
  if (!geometry) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "geometry is NULL");
  if (!out) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "out is NULL");
  long long voxels = 0;
  if (const int rc = occupancy_scalars(nullptr, geometry, z_scale, max_distance, &voxels); rc != MRS_TG_OK) return rc;
  mrs_tg::edtq::RegionPlan P;
  if (const int rc = field_region_plan(nullptr, geometry, z_scale, max_distance, region, &P); rc != MRS_TG_OK) return rc;
  for (int a = 0; a < 3; ++a) {
    out->reach[a] = P.reach[a];
    out->core_lo[a] = P.core_lo[a], out->core_hi[a] = P.core_hi[a];
    out->window_lo[a] = P.window_lo[a], out->window_hi[a] = P.window_hi[a];
  }
  out->whole_grid = P.whole_grid;
  out->workspace_bytes = (int64_t)P.workspace_doubles * (int64_t)sizeof(double);
  return MRS_TG_OK;
}

int mrs_tg_field_update_region(mrs_tg_ctx* ctx, const uint8_t* occupancy, const mrs_tg_field_geometry* geometry, double z_scale,
                               double max_distance, int32_t flags, const mrs_tg_field_region* region, void* workspace,
                               int64_t workspace_bytes, double* fields_inout) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  if (!geometry) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "geometry is NULL");
  long long voxels = 0;
  if (const int rc = occupancy_scalars(ctx, geometry, z_scale, max_distance, &voxels); rc != MRS_TG_OK) return rc;
  mrs_tg::edtq::RegionPlan P;
  if (const int rc = field_region_plan(ctx, geometry, z_scale, max_distance, region, &P); rc != MRS_TG_OK) return rc;
  if (const int rc = occupancy_arrays(ctx, voxels, flags, occupancy, fields_inout, "fields_inout_dev"); rc != MRS_TG_OK) return rc;
  if (!P.whole_grid) {
    const int64_t need = (int64_t)P.workspace_doubles * (int64_t)sizeof(double);
    if (!workspace) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "workspace_dev is NULL and %lld bytes are needed", (long long)need);
    if (((uintptr_t)workspace & 7u) != 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "workspace_dev is not 8-byte aligned");
    if (workspace_bytes < need)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "workspace_bytes = %lld is below the %lld bytes mrs_tg_field_update_query reports",
                  (long long)workspace_bytes, (long long)need);
    // (the bytes the kernels touch: `need` of them, whatever the caller's buffer holds beyond)
    const uintptr_t ws_lo = (uintptr_t)workspace, ws_hi = ws_lo + (size_t)need;
    if ((uintptr_t)occupancy < ws_hi && ws_lo < (uintptr_t)occupancy + (size_t)voxels)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "workspace_dev overlaps occupancy_dev");
    if ((uintptr_t)fields_inout < ws_hi && ws_lo < (uintptr_t)fields_inout + (size_t)voxels * sizeof(double))
      return fail(ctx, MRS_TG_ERR_INVALID_ARG, "workspace_dev overlaps fields_inout_dev");
  }
  const bool is_signed = (flags & MRS_TG_FIELD_SIGNED) != 0;
  const double h[3] = {geometry->spacing[0], geometry->spacing[1], geometry->spacing[2]};
  const int dims[3] = {geometry->dims[0], geometry->dims[1], geometry->dims[2]};
  HIP_TRY(ctx, use_device(ctx->device));
  ProfileScope ps(ctx, 41);
  HIP_TRY(ctx, mrs_tg::launch_field_update_region(occupancy, dims, region->field, P, mrs_tg::edtq::weights(h, z_scale),
                                                  mrs_tg::edtq::saturation(max_distance), max_distance, is_signed,
                                                  (double*)workspace, fields_inout, ctx->stream));
  return MRS_TG_OK;
}

// ---- one-call host interface ------------------------------------------------------------------


extern "C++" {
namespace mrs_tg {

void* ctx_host_scratch(mrs_tg_ctx* ctx, size_t bytes) {
  if (!ctx) return nullptr;
  // (a quarter more: a later round's arrays are a little larger, its paths have more waypoints)
  if (ctx->h_scratch.ensure(bytes, mrs_tg::PinnedAlloc::idle, bytes / 4) != hipSuccess) (void)hipGetLastError();
  return ctx->h_scratch.get();
}

}  // namespace mrs_tg
}  // extern "C++"

namespace {

struct SyncOnExit {  // nothing of a call is in flight when it returns, on error paths as well (the arenas are reused)
  hipStream_t st;
  ~SyncOnExit() { (void)hipStreamSynchronize(st); }
};

// device-side address of a host range the GPU can address as a whole: first AND last byte must be pinned and lie in the
// same mapping (a range that mrs_tg_host_register covers only in part, or an allocation shorter than the batch implies,
// takes the copying route -- where a short array is a host-side fault of the caller's, not a GPU page fault)
void* pinned_address(const void* ptr, size_t bytes) {
  auto query = [](const void* q, hipPointerAttribute_t* at) {
    if (hipPointerGetAttributes(at, q) != hipSuccess) {
      (void)hipGetLastError();  // an ordinary (pageable) pointer is reported as an error by some runtimes
      return false;
    }
    return at->type == hipMemoryTypeHost;
  };
  hipPointerAttribute_t first, last;
  if (!query(ptr, &first)) return nullptr;
  void* dev_first = first.devicePointer ? first.devicePointer : const_cast<void*>(ptr);
  if (bytes > 1) {
    const char* end = static_cast<const char*>(ptr) + (bytes - 1);
    if (!query(end, &last)) return nullptr;
    const char* dev_last = static_cast<const char*>(last.devicePointer ? last.devicePointer : (void*)end);
    if (dev_last - static_cast<const char*>(dev_first) != (ptrdiff_t)(bytes - 1)) return nullptr;  // two mappings
  }
  return dev_first;
}

}  // namespace

// the plan of the previous call is kept: the same batch shape again (a server's fixed batch, the re-solves of the nodelet's
// deviation loop) costs no analysis, no structure upload and no workspace allocation
static int cached_plan_for(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* so, mrs_tg_plan** plan_out) {
  mrs_tg_plan* plan = ctx->cached_plan;
  if (plan && (plan->view.n_paths != n_paths ||
               std::memcmp(plan->seg_offsets_host.data(), so, sizeof(int32_t) * ((size_t)n_paths + 1)) != 0)) {
    ctx->cached_plan = nullptr;
    mrs_tg_plan_destroy(plan);
    plan = nullptr;
  }
  if (!plan) {
    const int rc = mrs_tg_plan_create(ctx, n_paths, so, &plan);
    if (rc != MRS_TG_OK) return rc;
    ctx->cached_plan = plan;
  }
  *plan_out = plan;
  return MRS_TG_OK;
}

extern "C++" {
namespace mrs_tg {

// One round of optimize() for the `n_paths` requests still active: vertex expansion, findTrajectory's solve (one batched
// pipeline on the cached plan of this shape), both gates and validateTrajectorySpatial on the device.  `in.block` is the host
// block of policy_round_layout (pinned: read and written by the GPU in place through ONE copy kernel each way; pageable: by the
// runtime's copies); when the call returns its result region holds ok / n_samples / status / max_deviation / is_safe per
// path, the safe flag of every segment, and the sample rows of the paths that are finished.
int policy_round_device(mrs_tg_ctx* ctx, const PolicyRoundIn& in) {
  if (!ctx || !in.block || in.n_paths <= 0) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "policy round: nothing to solve");
  const size_t A = (size_t)in.n_paths, nS = in.n_segments, nV = in.n_vertices;
  const int cap = in.sample_capacity;
  const PolicyRoundLayout L = policy_round_layout(A, nS, cap);
  HIP_TRY(ctx, use_device(ctx->device));
  hipStream_t s = ctx->stream;
  mrs_tg_plan* plan = nullptr;
  int rc = cached_plan_for(ctx, in.n_paths, in.seg_offsets, &plan);
  if (rc != MRS_TG_OK) return rc;
  const PolicyRoundArena R = policy_round_arena(L, A, nS, cap);
  // (half as much again: the next round's paths have more waypoints -- one allocation for a request's rounds)
  HIP_TRY(ctx, ctx->d_arena.ensure(R.total_bytes, mrs_tg::StreamIdle{s}, R.total_bytes / 2));
  char* d = ctx->d_arena.get();
  SyncOnExit sync_on_exit{s};
  // is the whole block memory the GPU addresses (hipHostMalloc: ctx_host_scratch)?  Then one copy kernel moves the inputs,
  // and the results are written into it directly
  char* blk_dev = static_cast<char*>(pinned_address(in.block, L.total_bytes));
  const bool pinned = blk_dev != nullptr;
  if (pinned) {
    mrs_tg::CopyList upl;
    upl.add(blk_dev, d, L.in_bytes);
    HIP_TRY(ctx, mrs_tg::launch_copy_many(upl, s));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(d, in.block, L.in_bytes, hipMemcpyHostToDevice, s));
  }
  const double* wp_d = reinterpret_cast<const double*>(d + L.wp);
  uint8_t* mask_d = reinterpret_cast<uint8_t*>(d + R.mask);
  double* vals_d = reinterpret_cast<double*>(d + R.vals);
  HIP_TRY(ctx, mrs_tg::launch_policy_expand((int)nV, in.opt.derivative_to_optimize, wp_d, reinterpret_cast<const int32_t*>(d + L.vinfo),
                                            reinterpret_cast<const double*>(d + L.init), mask_d, vals_d, s));
  mrs_tg_options opt = in.opt;
  opt.estimate_times = 1;
  opt.sample_capacity = cap;
  // the length check below is the reference's answer to a runaway (:1178-1199) where its upper side runs; with that side off
  // the product's own runaway rule answers (MRS_TG_STATUS_ROUNDOFF_LIMITED: rejected by code), as on the host route
  if (in.max_len_factor > 0) opt.flags |= MRS_TG_FLAG_REFERENCE_STATUS;
  int32_t* st_d = reinterpret_cast<int32_t*>(d + R.status);
  int32_t* ns_d = reinterpret_cast<int32_t*>(d + R.n_samples);
  double* smp_d = reinterpret_cast<double*>(d + R.samples);
  // a moving start, as mrs_tg_solve_batch passes it on the host route (the launch shape of the outer loop depends on it:
  // launch_nonlinear); the round's builder read it off the initial states
  rc = plan_solve(plan, wp_d, mask_d, vals_d, reinterpret_cast<const double*>(d + L.lim), &opt, reinterpret_cast<double*>(d + R.times),
                  reinterpret_cast<double*>(d + R.coeffs), st_d, reinterpret_cast<double*>(d + R.cost), ns_d, smp_d,
                  in.moving_starts != 0);
  if (rc != MRS_TG_OK) return rc;
  // gates + validateTrajectorySpatial where the samples are; the small results go where the host reads them
  char* res = pinned ? blk_dev : d;  // (res + L.<field> addresses the field in either place: the arena mirrors the block)
  mrs_tg::PolicyValidateArgs va{};
  va.n_paths = in.n_paths;
  va.seg_offsets = reinterpret_cast<const int32_t*>(d + L.so);
  va.wp = wp_d;
  va.samples = smp_d;
  va.n_samples = ns_d;
  va.status = st_d;
  va.baca_total = reinterpret_cast<const double*>(d + L.baca);
  va.dt = opt.sampling_dt;
  va.max_len_factor = in.max_len_factor;
  va.min_len_factor = in.min_len_factor;
  va.max_deviation = in.max_deviation;
  va.capacity = cap;
  va.first_segment = in.first_segment;
  va.check_enabled = in.check_enabled;
  va.last_round = in.last_round;
  va.ok_out = reinterpret_cast<int32_t*>(res + L.ok);
  va.ns_out = reinterpret_cast<int32_t*>(res + L.ns);
  va.status_out = reinterpret_cast<int32_t*>(res + L.status);
  va.max_dev_out = reinterpret_cast<double*>(res + L.max_dev);
  va.is_safe_out = reinterpret_cast<uint8_t*>(res + L.is_safe);
  va.safe_out = reinterpret_cast<uint8_t*>(res + L.safe);
  va.ns_copy = reinterpret_cast<int32_t*>(d + R.rows);
  HIP_TRY(ctx, mrs_tg::launch_policy_validate(va, s));
  if (pinned) {  // the finished paths' rows only
    HIP_TRY(ctx, mrs_tg::launch_copy_samples(smp_d, reinterpret_cast<double*>(blk_dev + L.samples), va.ns_copy, in.n_paths, cap, s));
  } else {
    HIP_TRY(ctx, hipMemcpyAsync(in.block + L.ok, d + R.results, L.samples - L.ok, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(in.block + L.samples, smp_d, A * (size_t)cap * 4 * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(ctx, hipStreamSynchronize(s));
  return MRS_TG_OK;
}

}  // namespace mrs_tg
}  // extern "C++"

extern "C++" {
namespace {

using mrs_tg::A_WP, mrs_tg::A_MASK, mrs_tg::A_VALS, mrs_tg::A_LIM, mrs_tg::A_T;                // (the array table: mrs_tg_transfer.hpp)
using mrs_tg::A_C, mrs_tg::A_ST, mrs_tg::A_COST, mrs_tg::A_NS, mrs_tg::A_SMP, mrs_tg::A_COUNT;

// One call of the one-call interface between its plan and its kernels: the arrays (mrs_tg_transfer.hpp says how each one
// travels), their layout in the context's two arenas, and the steps that move them.
struct HostCall {
  mrs_tg_ctx* ctx;
  hipStream_t s;
  int32_t n_paths, sample_capacity;
  mrs_tg::TransferArray arr[A_COUNT];
  mrs_tg::TransferLayout lay;
  bool zero_copy = false;
  char* dbase() const { return ctx->d_arena.get(); }
  char* staged(int id) const { return ctx->h_arena.get() + lay.host_offset(arr[id]); }
  char* span(size_t device_offset) const { return ctx->h_arena.get() + (device_offset - lay.span_begin); }
  // where the kernels find array `id`: the caller's own (pinned) memory under zero copy, its slot of the arena otherwise
  template <class T>
  T* dev(int id) const {
    const mrs_tg::TransferArray& a = arr[id];
    return static_cast<T*>((zero_copy && a.pinned && a.bytes) ? a.pinned : static_cast<void*>(dbase() + a.off));
  }

  // grow-only, exactly what the largest call so far needed
  int ensure_arenas() {
    HIP_TRY(ctx, ctx->d_arena.ensure(lay.device_bytes, mrs_tg::StreamIdle{s}));
    HIP_TRY(ctx, ctx->h_arena.ensure(lay.host_bytes));
    return MRS_TG_OK;
  }

  // host to device: pinned arrays and the staged span in one copy kernel, large pageable arrays by the runtime
  int upload() const {
    if (zero_copy) return MRS_TG_OK;
    mrs_tg::CopyList up;
    bool listed = true;
    for (int id : mrs_tg::kUploadOrder) {
      const mrs_tg::TransferArray& a = arr[id];
      if (!a.src || !a.bytes) continue;
      if (a.staged) std::memcpy(staged(id), a.src, a.bytes);
      else if (a.pinned) listed = up.add(a.pinned, dbase() + a.off, a.bytes) && listed;
      else HIP_TRY(ctx, hipMemcpyAsync(dbase() + a.off, a.src, a.bytes, hipMemcpyHostToDevice, s));
    }
    if (lay.in_span_end > lay.span_begin)
      listed = up.add(span(lay.span_begin), dbase() + lay.span_begin, lay.in_span_end - lay.span_begin) && listed;
    if (!listed) return fail(ctx, MRS_TG_ERR_HIP, "more than %d copies in one upload", mrs_tg::kCopyMax);
    HIP_TRY(ctx, mrs_tg::launch_copy_many(up, s));
    return MRS_TG_OK;
  }

  // device to host, likewise; the staged outputs reach the caller in unpack_staged(), behind the synchronisation
  int download() const {
    if (zero_copy) return MRS_TG_OK;
    mrs_tg::CopyList down;
    bool listed = true;
    if (lay.span_end > lay.out_span_begin)
      listed = down.add(dbase() + lay.out_span_begin, span(lay.out_span_begin), lay.span_end - lay.out_span_begin);
    for (int id : mrs_tg::kDownloadOrder) {
      const mrs_tg::TransferArray& a = arr[id];
      if (!a.dst || !a.bytes || a.staged) continue;
      if (a.pinned && id == A_SMP)  // only the rows every path has produced (its capacity is sized for the longest acceptable one)
        HIP_TRY(ctx, mrs_tg::launch_copy_samples(dev<const double>(A_SMP), static_cast<double*>(a.pinned), dev<const int32_t>(A_NS),
                                                 n_paths, sample_capacity, s));
      else if (a.pinned) listed = down.add(dbase() + a.off, a.pinned, a.bytes) && listed;
      else HIP_TRY(ctx, hipMemcpyAsync(a.dst, dbase() + a.off, a.bytes, hipMemcpyDeviceToHost, s));
    }
    if (!listed) return fail(ctx, MRS_TG_ERR_HIP, "more than %d copies in one download", mrs_tg::kCopyMax);
    HIP_TRY(ctx, mrs_tg::launch_copy_many(down, s));
    return MRS_TG_OK;
  }

  void unpack_staged() const {
    if (zero_copy) return;
    for (int id : mrs_tg::kDownloadOrder)
      if (arr[id].dst && arr[id].bytes && arr[id].staged) std::memcpy(arr[id].dst, staged(id), arr[id].bytes);
  }
};

}  // namespace
}  // extern "C++"

static int solve_batch_impl(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* so, const double* wp, const uint8_t* mask,
                            const double* vals, const double* limits, const mrs_tg_options* opt, double* seg_times,
                            double* coeffs, int32_t* status, double* cost, int32_t* n_samples, double* samples,
                            bool coeffs_required) {
  // ---- check
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  int rc = check_options(ctx, opt);
  if (rc != MRS_TG_OK) return rc;
  if (!so || !mask || !vals || !seg_times || (!coeffs && coeffs_required) || !status)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "seg_offsets, fixed_mask, fixed_values, seg_times, coeffs_out, status_out are required");
  if (n_paths == 0) return MRS_TG_OK;
  const auto t_call = std::chrono::steady_clock::now();
  // ---- plan
  mrs_tg_plan* plan = nullptr;
  if ((rc = cached_plan_for(ctx, n_paths, so, &plan)) != MRS_TG_OK) return rc;
  // the caller's statement, checked on the host arrays (the offsets are valid behind the plan) before any array of the call
  // is uploaded or any kernel launched; mrs_tg_plan_bind_solve checks it on the device.  The kernels read positions from
  // either array, by the launch's size.  (Without the waypoints array the flag is refused by mrs_tg_plan_solve, as before.)
  if ((opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) && wp) {
    const long long bad = mrs_tg::count_position_mismatches_host(n_paths, so, wp, mask, vals);
    if (bad != 0)
      return fail(ctx, MRS_TG_ERR_INVALID_ARG,
                  "MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS: %lld vertices whose position constraint is absent or differs from their waypoint",
                  bad);
  }
  const size_t nS = (size_t)so[n_paths], nV = nS + (size_t)n_paths, P = (size_t)n_paths;
  const bool sampling = opt->sampling_dt > 0;
  if (sampling && !n_samples) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "n_samples_out is required when sampling");
  const size_t samp_doubles = sampling && samples ? P * (size_t)opt->sample_capacity * 4 : 0;
  HIP_TRY(ctx, use_device(ctx->device));
  HostCall call{ctx, ctx->stream, n_paths, opt->sample_capacity};

  // ---- classify and lay out (the table and the three ways an array travels: mrs_tg_transfer.hpp)
  // (the waypoints travel when something reads them: the time estimate, or kernels told that positions are the waypoints)
  const bool want_wp = wp != nullptr && (opt->estimate_times != 0 || (opt->flags & MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS) != 0);
  auto array = [stage_max = mrs_tg::knob::stage_max_bytes()](const void* src, void* dst, size_t bytes) {
    return mrs_tg::classify(src, dst, bytes, stage_max, pinned_address);
  };
  call.arr[A_WP] = array(want_wp ? wp : nullptr, nullptr, want_wp ? nV * 4 * sizeof(double) : 0);
  call.arr[A_MASK] = array(mask, nullptr, nV * 5);
  call.arr[A_VALS] = array(vals, nullptr, nV * 20 * sizeof(double));
  call.arr[A_LIM] = array(limits, nullptr, limits ? P * 9 * sizeof(double) : 0);
  call.arr[A_T] = array(seg_times, seg_times, nS * sizeof(double));
  call.arr[A_C] = array(nullptr, coeffs, nS * 40 * sizeof(double));
  call.arr[A_ST] = array(nullptr, status, P * sizeof(int32_t));
  call.arr[A_COST] = array(nullptr, cost, P * sizeof(double));
  call.arr[A_NS] = array(nullptr, sampling ? n_samples : nullptr, P * sizeof(int32_t));
  call.arr[A_SMP] = array(nullptr, samp_doubles ? samples : nullptr, samp_doubles * sizeof(double));
  call.lay = mrs_tg::lay_out(call.arr);
  // ---- ensure arenas
  if ((rc = call.ensure_arenas()) != MRS_TG_OK) return rc;
  SyncOnExit sync_on_exit{call.s};

  // ---- infer flags and the moving start the solve is told of: the masks are in host memory here.  A moving start matters to
  // the outer loop's launch shape only (small batches of 13-15 segments; launch_nonlinear)
  mrs_tg_options local = *opt;
  const mrs_tg::ConstraintScan scan = mrs_tg::scan_constraints(
      n_paths, so, mask, vals, local.derivative_to_optimize, !(local.flags & MRS_TG_FLAG_GENERAL_PATTERNS),
      !(local.flags & MRS_TG_FLAG_CONSTRAINED_SLOTS),
      mrs_tg::wants_moving_starts(local.time_alloc_method, (size_t)n_paths, plan->view.max_segments));
  if (scan.general_patterns) local.flags |= MRS_TG_FLAG_GENERAL_PATTERNS;
  if (scan.constrained_slots) local.flags |= MRS_TG_FLAG_CONSTRAINED_SLOTS;
  // ---- decide zero copy: one pass over every array (fixed times, default solve) and every array the caller passed is pinned
  call.zero_copy = mrs_tg::knob::zero_copy() && local.time_alloc_method == MRS_TG_TIME_ALLOC_NONE && !local.estimate_times &&
                   (local.flags & (MRS_TG_FLAG_GENERAL_PATTERNS | MRS_TG_FLAG_MATERIALIZED_BLOCKS)) == 0 &&
                   mrs_tg::rows_kernel_applies(plan->view, sampling) && (!sampling || mrs_tg::rows_tail_sampling_pays(plan->view)) &&
                   mrs_tg::every_array_pinned(call.arr);

  // ---- upload, deduct the spent budget, solve, download, synchronise, unpack
  if ((rc = call.upload()) != MRS_TG_OK) return rc;
  if (local.max_time_s > 0) {  // what is left of the caller's budget when the kernels start
    const double spent = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_call).count();
    local.max_time_s = local.max_time_s - spent > 1.0e-9 ? local.max_time_s - spent : 1.0e-9;
  }
  // (estimate_times without waypoints is refused by mrs_tg_plan_solve, as before)
  rc = plan_solve(plan, want_wp ? call.dev<double>(A_WP) : nullptr, call.dev<uint8_t>(A_MASK), call.dev<double>(A_VALS),
                  limits ? call.dev<double>(A_LIM) : nullptr, &local, call.dev<double>(A_T), call.dev<double>(A_C),
                  call.dev<int32_t>(A_ST), call.dev<double>(A_COST), sampling ? call.dev<int32_t>(A_NS) : nullptr,
                  samp_doubles ? call.dev<double>(A_SMP) : nullptr, scan.moving_starts);
  if (rc != MRS_TG_OK) return rc;
  if ((rc = call.download()) != MRS_TG_OK) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(call.s));
  call.unpack_staged();
  return MRS_TG_OK;
}

int mrs_tg_solve_batch(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* so, const double* wp, const uint8_t* mask,
                       const double* vals, const double* limits, const mrs_tg_options* opt, double* seg_times,
                       double* coeffs, int32_t* status, double* cost, int32_t* n_samples, double* samples) {
  return solve_batch_impl(ctx, n_paths, so, wp, mask, vals, limits, opt, seg_times, coeffs, status, cost, n_samples, samples, true);
}

extern "C++" {
namespace mrs_tg {
// mrs_tg_solve_batch for a caller that reads only the samples (the policy layer): the coefficients stay on the device
int solve_batch_samples_only(mrs_tg_ctx* ctx, int32_t n_paths, const int32_t* so, const double* wp, const uint8_t* mask,
                             const double* vals, const double* limits, const mrs_tg_options* opt, double* seg_times,
                             int32_t* status, int32_t* n_samples, double* samples) {
  return solve_batch_impl(ctx, n_paths, so, wp, mask, vals, limits, opt, seg_times, nullptr, status, nullptr, n_samples, samples,
                          false);
}
}  // namespace mrs_tg
}  // extern "C++"

// Pinned host memory for the arrays of mrs_tg_solve_batch / mrs_tg_optimize_paths: buffers allocated (or registered) here
// are read and written by the GPU's DMA engines directly, with no staging copy on either side.
int mrs_tg_host_alloc(size_t bytes, void** ptr_out) {
  if (!ptr_out) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ptr_out is NULL");
  *ptr_out = nullptr;
  const hipError_t e = hipHostMalloc(ptr_out, bytes ? bytes : 8, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, e == hipErrorOutOfMemory ? MRS_TG_ERR_NOMEM : MRS_TG_ERR_HIP, "hipHostMalloc(%zu) failed: %s", bytes,
                hipGetErrorString(e));
  }
  return MRS_TG_OK;
}

void mrs_tg_host_free(void* ptr) {
  if (ptr) (void)hipHostFree(ptr);
}

int mrs_tg_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "nothing to register");
  const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, MRS_TG_ERR_HIP, "hipHostRegister failed: %s", hipGetErrorString(e));
  }
  return MRS_TG_OK;
}

int mrs_tg_host_unregister(void* ptr) {
  if (!ptr) return MRS_TG_OK;
  const hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, MRS_TG_ERR_HIP, "hipHostUnregister failed: %s", hipGetErrorString(e));
  }
  return MRS_TG_OK;
}

// ---- single path, findTrajectory()'s signature -------------------------------------------------


int mrs_tg_find_trajectory(mrs_tg_ctx* ctx, const mrs_tg_waypoint* wps, int32_t n_wp, const mrs_tg_initial_state* init,
                           const double* limits9, const mrs_tg_options* opt_in, int32_t relax_heading,
                           double* seg_times_out, double* coeffs_out, int32_t* status_out, int32_t* n_samples_out,
                           double* samples_out) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  if (!wps || !limits9 || !opt_in || !seg_times_out || !coeffs_out || !status_out || !n_samples_out)
    return fail(ctx, MRS_TG_ERR_INVALID_ARG, "NULL argument");
  if (n_wp < 2) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "need at least 2 waypoints, got %d", n_wp);
  const int d = opt_in->derivative_to_optimize;
  if (d < 2 || d > 4) return fail(ctx, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize must be 2, 3 or 4");
  namespace pol = mrs_tg::policy;
  const int V = n_wp, S = n_wp - 1;
  ctx->find_rejection = MRS_TG_FIND_ACCEPTED;
  ctx->find_baca_total = 0.0;
  *n_samples_out = 0;
  try {
    std::vector<double> raw(V * 4), wp(V * 4), vals(V * 20), baca;
    std::vector<uint8_t> mask(V * 5), stop(V);
    for (int i = 0; i < V; ++i) {
      for (int k = 0; k < 4; ++k) raw[i * 4 + k] = wps[i].coords[k];
      stop[i] = wps[i].stop_at;
    }
    // vertices: src/mrs_trajectory_generation.cpp:923-977; limits: :985-1038
    pol::build_vertices(raw.data(), stop.data(), V, init, d, wp.data(), mask.data(), vals.data());
    double lim[9];
    pol::effective_limits(limits9, relax_heading != 0, lim);
    // initial_total_time_baca (:1048-1056), from the same vertices and limits the optimiser sees
    ctx->find_baca_total = pol::baca_total_time(S, wp.data(), lim, baca);
    mrs_tg_options opt = *opt_in;
    opt.estimate_times = 1;
    // the reference's own status rule: a runaway of the feasibility scaling keeps the outer loop's code and is discarded by
    // the length check below, as at :1178-1199 (a 5 cm path whose estimate is 0.025 s is no runaway: it is never checked) --
    // where the upper side of that check really runs.  Without sampling, or with that side switched off (a factor <= 0: the
    // reference has no such switch), the product's own runaway rule answers: MRS_TG_STATUS_ROUNDOFF_LIMITED, rejected by code
    if (opt_in->sampling_dt > 0 && samples_out && opt_in->max_trajectory_len_factor > 0) opt.flags |= MRS_TG_FLAG_REFERENCE_STATUS;
    const int32_t so[2] = {0, S};
    double cost = 0.0;
    int rc = mrs_tg_solve_batch(ctx, 1, so, wp.data(), mask.data(), vals.data(), lim, &opt, seg_times_out, coeffs_out,
                                status_out, &cost, n_samples_out, samples_out);
    if (rc != MRS_TG_OK) return rc;
  } catch (const std::bad_alloc&) {
    return fail(ctx, MRS_TG_ERR_NOMEM, "out of host memory for a path of %d waypoints", n_wp);
  }
  // accept >= 1 except MAXTIME(6), and -1 (src/mrs_trajectory_generation.cpp:1138-1149)
  if (!mrs_tg::baca::code_accepted(*status_out)) {
    ctx->find_rejection = MRS_TG_FIND_REJECTED_CODE;
    ctx->last_error = "optimization failed with code " + std::to_string(*status_out);
    *n_samples_out = 0;
    return MRS_TG_OK;
  }
  // "validate the temporal sampling of the trajectory" (:1178-1199): states.size() * sampling_dt against the Baca total.  A
  // trajectory with more samples than samples_out holds is reported as capacity + 1: the count the check sees is then a
  // LOWER bound of the real one, enough to reject "too long" whenever capacity * dt exceeds the allowed length -- and no
  // ground for "too short": the lower side is skipped for it
  if (opt_in->sampling_dt > 0 && samples_out) {
    const bool overflowed = *n_samples_out > opt_in->sample_capacity;
    const int verdict = mrs_tg::baca::length_check(*n_samples_out, opt_in->sampling_dt, ctx->find_baca_total,
                                                   opt_in->max_trajectory_len_factor,
                                                   overflowed ? 0.0 : opt_in->min_trajectory_len_factor);
    if (verdict != 0) {
      char msg[256];
      std::snprintf(msg, sizeof(msg), "trajectory sampling failed: the final trajectory sampling is too %s = %.2f, initial 'baca' "
                    "estimate = %.2f, allowed factor %.2f", verdict > 0 ? "long" : "short", *n_samples_out * opt_in->sampling_dt,
                    ctx->find_baca_total, verdict > 0 ? opt_in->max_trajectory_len_factor : opt_in->min_trajectory_len_factor);
      ctx->last_error = msg;
      ctx->find_rejection = verdict > 0 ? MRS_TG_FIND_REJECTED_TOO_LONG : MRS_TG_FIND_REJECTED_TOO_SHORT;
      *n_samples_out = 0;
    }
  }
  return MRS_TG_OK;
}

int mrs_tg_find_trajectory_info(const mrs_tg_ctx* ctx, int32_t* rejection_out, double* baca_total_time_out) {
  if (!ctx) return fail(nullptr, MRS_TG_ERR_INVALID_ARG, "ctx is NULL");
  if (rejection_out) *rejection_out = ctx->find_rejection;
  if (baca_total_time_out) *baca_total_time_out = ctx->find_baca_total;
  return MRS_TG_OK;
}

}  // extern "C"

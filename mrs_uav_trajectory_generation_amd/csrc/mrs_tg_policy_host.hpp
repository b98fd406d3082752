// mrs_tg_policy_host.hpp -- the PURE-HOST half of the path-policy layer: what MrsTrajectoryGeneration::optimize() does around
// findTrajectory() (/root/reference/src/mrs_trajectory_generation.cpp:620-851), for a batch of independent paths, with the
// solver behind a callback:
//   preprocessPath (:431-500) -> vertices as findTrajectory builds them (:923-977) -> host.solve(all active paths of the
//   round) -> nlopt-code gate (:1138-1149) -> length sanity check against the Baca estimate (:1048-1056, :1178-1199) ->
//   validateTrajectorySpatial (:1401-1455) -> mid-points into unsafe segments (:739-753) -> next round; optional
//   findTrajectoryFallback (:1215-1395) and override_heading_atan2 (:1582-1597).
// The arithmetic shared with the plan steps -- distance from a segment, the validation scan, the gates, the waypoint hit test,
// the Baca estimate, thinning and mid-points, the vertex rule and the limits' tail, the heading unwrap, the yaw round trip and
// the fallback's rows, the direction-of-travel rule -- is not written here: it is called from the host-checkable kernel headers
// (mrs_tg_deviation.hpp, mrs_tg_passage.hpp, mrs_tg_baca.hpp, mrs_tg_pathedit.hpp, mrs_tg_request.hpp, mrs_tg_fallback.hpp,
// mrs_tg_heading.hpp), which policy_validate_kernel, policy_expand_kernel and the plan steps' kernels call too.
// No HIP type or call appears here: mrs_tg_policy.hip instantiates optimize_paths() with the batched GPU solve and
// mrs_tg_abi.hip's mrs_tg_find_trajectory uses the vertex builder, the Baca total and the two gates; the same header compiles
// with g++ and is driven by tests/host/policy_host_harness.cpp with the CPU oracle as the solver on 16 threads under
// ASan / UBSan / TSan (tests/test_host_sanitizers.py).  Tf has no counterpart; the initial condition of stamped paths ("path
// from the future", before takeoff) and the MPC prediction splice happen around this layer, in include/mrs_tg_initial_condition.hpp.
#pragma once

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <stdexcept>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include <sched.h>

#include "../../include/mrs_tg.h"
#include "mrs_tg_baca.hpp"
#include "mrs_tg_fallback.hpp"
#include "mrs_tg_heading.hpp"
#include "mrs_tg_knobs.hpp"
#include "mrs_tg_passage.hpp"
#include "mrs_tg_pathedit.hpp"
#include "mrs_tg_request.hpp"
#include "mrs_tg_transfer.hpp"

struct mrs_tg_ctx;

namespace mrs_tg {

// ---- one round of the policy loop on the device (mrs_tg_abi.hip::policy_round_device, kernels in mrs_tg_policy_dev.hip) ----
// The host block of a round: inputs | results, every field 256-byte aligned.  Plain arithmetic, shared by the host code that
// fills / reads the block and the device code that mirrors it in its arena.
struct PolicyRoundLayout {
  size_t wp, init, lim, baca, vinfo, so, in_bytes;                      // inputs (offsets in the block)
  size_t ok, ns, status, max_dev, is_safe, safe, samples, total_bytes;   // results
};
inline PolicyRoundLayout policy_round_layout(size_t A, size_t nS, int32_t capacity) {
  constexpr auto up = align_slot;
  const size_t nV = nS + A;
  PolicyRoundLayout L{};
  size_t off = 0;
  L.wp = off, off += up(nV * 4 * sizeof(double));          // unwrapped waypoints [vertex][4]
  L.init = off, off += up(A * reqq::kState * sizeof(double));  // the initial state as reqq reads it [path][4][4] (state_rows)
  L.lim = off, off += up(A * 9 * sizeof(double));          // limits after relax_heading [path][9]
  L.baca = off, off += up(A * sizeof(double));             // initial_total_time_baca [path]
  L.vinfo = off, off += up(nV * sizeof(int32_t));          // position of the vertex's path << 4 | kVertex* flags
  L.so = off, off += up((A + 1) * sizeof(int32_t));        // segment offsets
  L.in_bytes = off;
  L.ok = off, off += up(A * sizeof(int32_t));              // both gates passed (and the samples fit)
  L.ns = off, off += up(A * sizeof(int32_t));
  L.status = off, off += up(A * sizeof(int32_t));
  L.max_dev = off, off += up(A * sizeof(double));
  L.is_safe = off, off += up(A);
  L.safe = off, off += up(nS ? nS : 1);                    // validateTrajectorySpatial's flag of every segment
  L.samples = off, off += up(A * (size_t)capacity * 4 * sizeof(double));  // rows of the FINISHED paths only
  L.total_bytes = off;
  return L;
}
// The device arena of the same round: [the block's input region] | results, laid out as in the block up to its samples |
// what the solve reads and writes | the rows to copy per path | samples.  (arena + a.results - L.in_bytes + L.<result field>
// is the field's mirror: a.results == L.in_bytes.)
struct PolicyRoundArena {
  size_t results, mask, vals, times, coeffs, cost, status, n_samples, rows, samples, total_bytes;
};
inline PolicyRoundArena policy_round_arena(const PolicyRoundLayout& L, size_t A, size_t nS, int32_t capacity) {
  constexpr auto up = align_slot;
  const size_t nV = nS + A;
  PolicyRoundArena a{};
  size_t off = L.in_bytes;
  a.results = off, off += L.samples - L.in_bytes;
  a.mask = off, off += up(nV * 5);
  a.vals = off, off += up(nV * 20 * sizeof(double));
  a.times = off, off += up(nS * sizeof(double));
  a.coeffs = off, off += up(nS * 40 * sizeof(double));
  a.cost = off, off += up(A * sizeof(double));
  a.status = off, off += up(A * sizeof(int32_t));
  a.n_samples = off, off += up(A * sizeof(int32_t));
  a.rows = off, off += up(A * sizeof(int32_t));               // min(n_samples, capacity) of the finished paths, 0 otherwise
  a.samples = off, off += up(A * (size_t)capacity * 4 * sizeof(double));
  a.total_bytes = off;
  return a;
}
constexpr int kVertexFirst = 1, kVertexLast = 2, kVertexStop = 4, kVertexInit = 8;
struct PolicyRoundIn {
  int32_t n_paths;
  const int32_t* seg_offsets;  // [n_paths + 1] (host; also at block + layout.so)
  size_t n_segments, n_vertices;
  char* block;                 // policy_round_layout(n_paths, n_segments, sample_capacity).total_bytes
  mrs_tg_options opt;
  double max_len_factor, min_len_factor, max_deviation;
  int32_t first_segment, check_enabled, last_round, sample_capacity;
  // a request of the round starts from a moving state (a non-zero velocity / acceleration / jerk of its initial state): what
  // scan_constraints reads off the expanded vertices on the host route.  Wanted, and therefore set, only for the shapes whose
  // outer-loop launch depends on it (wants_moving_starts, mrs_tg_transfer.hpp)
  int32_t moving_starts;
};
int policy_round_device(::mrs_tg_ctx* ctx, const PolicyRoundIn& in);  // (defined in mrs_tg_abi.hip: the GPU build only)

namespace policy {

using pathq::interpolate_point;  // :1612-1625

// estimateSegmentTimesBaca, /root/reference/src/eth_trajectory_generation/vertex.cpp:301-485; wp [V][4] unwrapped
inline void estimate_times_baca(int S, const double* wp, const double* lim, std::vector<double>& out) {
  out.resize(S > 0 ? S : 0);
  const baca::Thresholds th = baca::thresholds(lim);
  for (int i = 0; i < S; ++i) out[i] = baca::classify(wp, i, S, lim, th).value;
}

// The policy's per-path host work (vertex building, Baca estimates, spatial validation, mid-point insertion) is independent
// from path to path: batches of requests run it on a few threads.  Ranges of [0, n) in order, one per thread; small batches
// (a nodelet's single request) stay on the calling thread.  MRS_TG_POLICY_THREADS=1 switches the threads off.
inline int policy_threads() {
  static const int n = [] {
    if (knob::policy_threads()) return knob::policy_threads();
    int cpus = (int)std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof(set), &set) == 0) cpus = std::min(cpus > 0 ? cpus : 1 << 20, CPU_COUNT(&set));
    return std::max(1, std::min(cpus, 16));
  }();
  return n;
}

// body(begin, end) over ranges of [0, n).  An exception thrown by any range (std::bad_alloc from a worker's vectors) is
// caught on the thread that raised it, every thread is joined, and the FIRST exception is rethrown on the calling thread --
// nothing escapes a std::thread (which would be std::terminate) and no joinable thread is ever destroyed.
template <class F>
void parallel_ranges(size_t n, size_t min_per_thread, F&& body) {
  // MRS_TG_POLICY_GRAIN=k (test knob, read once): k items are enough for a thread, whatever the call site asks for -- lets a
  // test put a few dozen requests on 16 threads (tests/host/policy_host_harness.cpp)
  if (knob::policy_grain()) min_per_thread = knob::policy_grain();
  const size_t threads = std::min<size_t>((size_t)policy_threads(), n / std::max<size_t>(min_per_thread, 1));
  if (threads <= 1) {
    body((size_t)0, n);
    return;
  }
  const size_t chunk = (n + threads - 1) / threads;
  std::vector<std::exception_ptr> raised(threads);   // slot t: what range t threw (written by one thread each)
  auto guarded = [&body, &raised](size_t t, size_t b, size_t e) noexcept {
    try {
      body(b, e);
    } catch (...) {
      raised[t] = std::current_exception();
    }
  };
  struct Joiner {   // joins on every way out of this scope
    std::vector<std::thread> pool;
    ~Joiner() {
      for (std::thread& th : pool)
        if (th.joinable()) th.join();
    }
  } joiner;
  size_t first_inline = threads;  // ranges [first_inline, threads) run on this thread: a thread that could not be started
  try {
    joiner.pool.reserve(threads - 1);
    for (size_t t = 1; t < threads; ++t) {
      const size_t b = std::min(n, t * chunk), e = std::min(n, b + chunk);
      if (b >= e) continue;
      try {
        joiner.pool.emplace_back(guarded, t, b, e);
      } catch (const std::system_error&) {
        first_inline = t;
        break;
      }
    }
  } catch (const std::bad_alloc&) {  // (the pool's own vector): everything not started runs here
    first_inline = joiner.pool.size() + 1;
  }
  guarded(0, (size_t)0, std::min(n, chunk));
  for (size_t t = first_inline; t < threads; ++t) {
    const size_t b = std::min(n, t * chunk), e = std::min(n, b + chunk);
    if (b < e) guarded(t, b, e);
  }
  for (std::thread& th : joiner.pool) th.join();
  for (const std::exception_ptr& ex : raised)
    if (ex) std::rethrow_exception(ex);
}

struct PathState {
  std::vector<double> wps;     // [n][4] current waypoints (raw headings)
  std::vector<uint8_t> stop;
  int n_wp = 0;
  bool done = false, ok = false;
  int n_samples = 0, iterations = 0;
  double max_dev = 0.0;
  double baca_total = 0.0;
};

// the thinning decision is pathq::keeps (mrs_tg_pathedit.hpp), which thin_path_kernel calls too
inline void preprocess(const mrs_tg_waypoint* in, int n_in, const mrs_tg_policy_options& o, PathState& st) {  // :431-500
  st.wps.clear();
  st.stop.clear();
  static_assert(sizeof(mrs_tg_waypoint) % sizeof(double) == 0 && offsetof(mrs_tg_waypoint, coords) == 0, "rows of doubles");
  const size_t stride = sizeof(mrs_tg_waypoint) / sizeof(double);
  const double* rows = reinterpret_cast<const double*>(in);  // x, y, z, heading in front of every `stride` doubles
  const pathq::ThinOptions thin{o.min_waypoint_distance, o.path_straightener_enabled, o.path_straightener_max_deviation,
                                o.path_straightener_max_hdg_deviation};
  int last_added = 0;
  for (int i = 0; i < n_in; ++i) {
    if (!pathq::keeps(rows, stride, n_in, last_added, i, thin)) continue;
    const double* w = in[i].coords;
    st.wps.insert(st.wps.end(), w, w + 4);
    st.stop.push_back(in[i].stop_at);
    last_added = i;
  }
  st.n_wp = (int)st.stop.size();
}

// validateTrajectorySpatial :1401-1455
inline bool validate_spatial(const double* samples, int n_samples, const PathState& st, const mrs_tg_policy_options& o,
                      std::vector<uint8_t>& safe, double& max_dev) {
  safe.resize(std::max(st.n_wp - 1, 0));
  const devq::Validation v = devq::validate(samples, n_samples, st.wps.data(), st.n_wp, o.max_deviation_first_segment,
                                            o.max_deviation, safe.data());
  max_dev = v.max_deviation;
  return v.is_safe;
}

inline void insert_midpoints(PathState& st, const std::vector<uint8_t>& safe, const mrs_tg_policy_options& o) {  // :739-753
  const int V = st.n_wp;  // (the reference tests the size where nothing has been inserted yet: pathq::inserts)
  int w = 0, sidx = 0;
  while (w < st.n_wp - 1) {
    if (pathq::inserts(!safe[sidx], sidx, o.max_deviation_first_segment, V)) {
      double mid[4];
      interpolate_point(st.wps.data() + (size_t)w * 4, st.wps.data() + (size_t)(w + 1) * 4, 0.5, mid);
      st.wps.insert(st.wps.begin() + (size_t)(w + 1) * 4, mid, mid + 4);
      st.stop.insert(st.stop.begin() + (w + 1), (uint8_t)0);
      ++st.n_wp;
      ++w;
    }
    ++sidx;
    ++w;
  }
}

// findTrajectoryFallback :1215-1395: the rows are fbq's (mrs_tg_fallback.hpp), which fallback_sample_kernel runs too.  Returns
// the number of rows, also where it exceeds the capacity (the rows below the capacity are written)
inline int fallback_sampling(const PathState& st, const double* limits9, bool relax_heading, const mrs_tg_policy_options& o, double dt,
                      double* out, int capacity) {
  const int S = st.n_wp - 1;
  std::vector<double> wps(st.wps.size());
  fbq::unwrap_path(st.wps.data(), st.n_wp, wps.data());
  double lim[9];
  std::memcpy(lim, limits9, sizeof(lim));
  // (reqq::limits relaxes first and scales second, as the reference does: the two steps touch disjoint entries, the order cannot show)
  reqq::scale_fallback_limits(lim, o.fallback_speed_factor, o.fallback_accel_factor);
  if (relax_heading) reqq::relax_heading_limits(lim);
  std::vector<double> t_baca;
  estimate_times_baca(S, wps.data(), lim, t_baca);
  int32_t insert = 0;
  // a stopping time that gives no dwell a path can have (negative, not a number, beyond int32) gives no trajectory, as the
  // plan step refuses it: more rows than fit
  const bool dwell_ok = fbq::insert_count(o.fallback_stopping_time, dt, &insert);
  long long count = dwell_ok ? 0 : (long long)capacity + 1;  // 64-bit until it is returned
  for (int i = 0; dwell_ok && i < S; ++i) {
    const fbq::SegmentRows seg = fbq::segment_rows(t_baca[i], dt, insert, i, S, st.stop[i] != 0);
    const double* a = st.wps.data() + (size_t)i * 4;  // (the rows interpolate the RAW headings, :1362)
    for (long long r = 0; r < seg.rows && count + r < capacity; ++r)
      fbq::row_at(a, a + 4, fbq::row_coeff(seg.nd, seg.dwell, r), out + (size_t)(count + r) * 4);
    count += seg.rows;
  }
  return (int)std::min<long long>(count, INT_MAX);
}

// ---- the single-path seam: the pieces of findTrajectory() around the solver -------------------------------------------

// the limits findTrajectory hands to the estimators and the optimiser: relax_heading lifts the heading limits (:1030-1038)
inline void effective_limits(const double* limits9, bool relax_heading, double* lim_out) {
  for (int k = 0; k < 9; ++k) lim_out[k] = limits9[k];
  if (relax_heading) reqq::relax_heading_limits(lim_out);
}

// an initial state as the [4][4] rows reqq reads: row 0 column 3 the heading, rows 1 .. 3 velocity, acceleration, jerk; a null
// state gives zeros (and is not read by a path that has none)
inline void state_rows(const mrs_tg_initial_state* init, double* state) {
  for (int e = 0; e < reqq::kState; ++e) state[e] = 0.0;
  if (!init) return;
  state[3] = init->heading;
  for (int k = 0; k < 4; ++k) state[4 + k] = init->velocity[k], state[8 + k] = init->acceleration[k], state[12 + k] = init->jerk[k];
}

// The vertices findTrajectory builds for one path (:923-977) are reqq::vertices (mrs_tg_request.hpp): this is the call from
// the ABI's types.  wps_raw [n_wp][4] raw headings; wp_out [n_wp][4], mask_out [n_wp][5], vals_out [n_wp][5][4], each or null.
inline void build_vertices(const double* wps_raw, const uint8_t* stop_at, int n_wp, const mrs_tg_initial_state* init, int d,
                           double* wp_out, uint8_t* mask_out, double* vals_out) {
  double state[reqq::kState];
  state_rows(init, state);
  reqq::vertices(wps_raw, stop_at, n_wp, init != nullptr, state, d, wp_out, mask_out, vals_out);
}

// initial_total_time_baca (:1048-1056): the sum of estimateSegmentTimesBaca over the path's vertices
inline double baca_total_time(int n_seg, const double* wp_unwrapped, const double* lim, std::vector<double>& scratch) {
  estimate_times_baca(n_seg, wp_unwrapped, lim, scratch);
  double tot = 0;
  for (double t : scratch) tot += t;
  return tot;
}

// a Host with `int round(const PolicyRoundIn&)` and `bool device_round_enabled(size_t active_paths)` runs the rounds' batch-sized work on the device
template <class H, class = void>
struct HasDeviceRound : std::false_type {};
template <class H>
struct HasDeviceRound<H, std::void_t<decltype(&H::round)>> : std::true_type {};

template <class Host, class... Args>
int failf(Host& host, int code, const char* fmt, Args... args) {
  char buf[256];
  std::snprintf(buf, sizeof(buf), fmt, args...);
  return host.fail(code, buf);
}

// optimize() (:620-851) for n_paths independent requests.  Host supplies
//   void* scratch(size_t bytes)            a block the solver reads / writes cheaply (pinned), or nullptr: ordinary memory
//   int solve(A, seg_offsets, waypoints, mask, values, limits, &options, times, status, n_samples, samples)
//                                          mrs_tg_solve_batch's contract for the round's A active paths (samples only)
//   int fail(code, message)                records the message, returns the code
// May throw std::bad_alloc (the callers map it to MRS_TG_ERR_NOMEM).
template <class Host>
int optimize_paths(Host& host, int32_t n_paths, const int32_t* wp_offsets, const mrs_tg_waypoint* waypoints,
                   const mrs_tg_initial_state* initial_states, const uint8_t* has_initial_state, const double* limits,
                   const uint8_t* relax_heading, const mrs_tg_policy_options* opt, int32_t sample_capacity,
                   int32_t* success_out, int32_t* n_samples_out, double* samples_out, double* max_deviation_out,
                   int32_t* n_waypoints_out, int32_t* iterations_out) {
  if (!wp_offsets || !waypoints || !limits || !opt || !success_out || !n_samples_out || !samples_out)
    return host.fail(MRS_TG_ERR_INVALID_ARG, "wp_offsets, waypoints, limits, options, success_out, n_samples_out and samples_out are required");
  if (n_paths < 0 || sample_capacity <= 0)
    return failf(host, MRS_TG_ERR_INVALID_ARG, "n_paths %d / sample_capacity %d: need >= 0 / > 0", n_paths, sample_capacity);
  const mrs_tg_policy_options& o = *opt;
  const int d = o.solver.derivative_to_optimize;
  if (d < 2 || d > 4)
    return failf(host, MRS_TG_ERR_INVALID_ARG, "derivative_to_optimize must be 2, 3 or 4 (got %d)", d);
  const double dt = o.solver.sampling_dt;
  if (!(dt > 0)) return failf(host, MRS_TG_ERR_INVALID_ARG, "the policy layer needs sampling_dt > 0 (got %g)", dt);
  const auto t_begin = std::chrono::steady_clock::now();
  auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(); };
  std::vector<PathState> st((size_t)n_paths);
  parallel_ranges((size_t)n_paths, 256, [&](size_t p0, size_t p1) {
    for (size_t p = p0; p < p1; ++p) {
      preprocess(waypoints + wp_offsets[p], wp_offsets[p + 1] - wp_offsets[p], o, st[p]);
      if (st[p].n_wp <= 1) {  // "the path is empty (after postprocessing)" :676-681
        st[p].done = true;
        st[p].ok = false;
      }
    }
  });
  std::vector<int> active;
  // MRS_TG_POLICY_TRACE=1: where the call's time went (host phases and the batched GPU call), on stderr
  const bool trace = knob::policy_trace();
  double t_build = 0, t_solve = 0, t_post = 0, t_validate = 0;
  auto now = [&]() { return trace ? elapsed() : 0.0; };
  for (int round = 0; round <= o.max_deviation_iterations; ++round) {
    active.clear();
    for (int p = 0; p < n_paths; ++p)
      if (!st[p].done) active.push_back(p);
    if (active.empty()) break;
    // optimize() picks the solver of a round in this order (:702-716, :754-768): fallback sampling when it was asked for,
    // fallback sampling when overtime() says the request is running late ("executing fallback sampling, we are running
    // over time" -- the request still succeeds), else findTrajectory.  Only the checks BEHIND the solve (:1085, :1156,
    // :1171, :1516-1522) give a request up.
    double budget_left = 0.0;  // timeLeft() :1749-1761
    auto overtime = [&]() {    // overtime() :1730-1743 (OVERTIME_SAFETY_FACTOR 0.95, OVERTIME_SAFETY_OFFSET 0.01 s)
      return o.max_execution_time_s > 0 && elapsed() > 0.95 * o.max_execution_time_s - 0.01;
    };
    bool use_fallback = o.fallback_sampling != 0;
    if (!use_fallback && o.max_execution_time_s > 0) {
      const double spent = elapsed();
      budget_left = spent >= o.max_execution_time_s ? 0.0 : o.max_execution_time_s - spent;
      use_fallback = overtime();
    }
    // the requests are independent: one that cannot be solved (its deviation loop has subdivided it beyond the longest
    // path a plan takes; the reference has no such limit) fails on its own and leaves the others alone
    if (!use_fallback) {
      size_t kept = 0;
      for (int p : active) {
        if (st[p].n_wp - 1 > MRS_TG_MAX_SEGMENTS) {
          st[p].done = true;
          st[p].ok = false;
          st[p].n_samples = 0;
        } else {
          active[kept++] = p;
        }
      }
      active.resize(kept);
      if (active.empty()) break;
    }
    // ---- a host that runs the round on the device (the GPU build): vertices expanded, gates and validateTrajectorySpatial
    // applied where the samples are; the waypoints travel up, a few words per path and the FINISHED paths' samples come down
    if constexpr (HasDeviceRound<Host>::value) {
      if (!use_fallback && host.device_round_enabled(active.size())) {
        const double t0 = now();
        const size_t A = active.size();
        std::vector<int32_t> so(A + 1, 0);
        for (size_t a = 0; a < A; ++a) so[a + 1] = so[a] + st[active[a]].n_wp - 1;
        const size_t nS = (size_t)so.back(), nV = nS + A;
        const PolicyRoundLayout L = policy_round_layout(A, nS, sample_capacity);
        char* block = knob::policy_pinned() ? static_cast<char*>(host.scratch(L.total_bytes)) : nullptr;
        std::vector<char> pageable;
        if (!block) {
          pageable.resize(L.total_bytes);
          block = pageable.data();
        }
        double* wp = reinterpret_cast<double*>(block + L.wp);
        double* init = reinterpret_cast<double*>(block + L.init);
        double* lim = reinterpret_cast<double*>(block + L.lim);
        double* baca = reinterpret_cast<double*>(block + L.baca);
        int32_t* vinfo = reinterpret_cast<int32_t*>(block + L.vinfo);
        std::memcpy(block + L.so, so.data(), sizeof(int32_t) * (A + 1));
        bool any_stop = false;
        for (size_t a = 0; a < A && !any_stop; ++a)
          for (int i = 1; i + 1 < st[active[a]].n_wp && !any_stop; ++i) any_stop = st[active[a]].stop[i] != 0;
        // the moving-start hint of this round's solve: mrs_tg_solve_batch reads it off the vertices (scan_constraints), which
        // exist on the device only here -- a first vertex constrains exactly the initial state's velocity, acceleration and jerk
        int max_segments = 0;
        for (size_t a = 0; a < A; ++a) max_segments = std::max(max_segments, (int)(so[a + 1] - so[a]));
        bool moving_starts = false;
        if (wants_moving_starts(o.solver.time_alloc_method, A, max_segments) && has_initial_state && initial_states)
          for (size_t a = 0; a < A && !moving_starts; ++a) {
            const int p = active[a];
            if (!has_initial_state[p]) continue;
            for (int k = 0; k < 4; ++k)
              moving_starts = moving_starts || initial_states[p].velocity[k] != 0.0 || initial_states[p].acceleration[k] != 0.0 ||
                              initial_states[p].jerk[k] != 0.0;
          }
        parallel_ranges(A, 128, [&](size_t a0, size_t a1) {
          std::vector<double> tb;
          for (size_t a = a0; a < a1; ++a) {
            const int p = active[a];
            const PathState& s = st[p];
            const bool has_init = has_initial_state && has_initial_state[p] && initial_states;
            const size_t v0 = (size_t)so[a] + a;
            // the unwrapped waypoints only (:925-936): mask and values are expanded on the device, from vinfo and the state rows
            double* state = init + a * reqq::kState;
            state_rows(has_init ? &initial_states[p] : nullptr, state);
            reqq::vertices(s.wps.data(), nullptr, s.n_wp, has_init, state, d, wp + v0 * 4, nullptr, nullptr);
            for (int i = 0; i < s.n_wp; ++i)
              vinfo[v0 + i] = (int32_t)(a << 4) | (i == 0 ? kVertexFirst : 0) | (i == s.n_wp - 1 ? kVertexLast : 0) |
                              ((i > 0 && i < s.n_wp - 1 && s.stop[i]) ? kVertexStop : 0) | ((i == 0 && has_init) ? kVertexInit : 0);
            effective_limits(limits + (size_t)p * 9, relax_heading && relax_heading[p], lim + a * 9);
            st[p].baca_total = baca[a] = baca_total_time(s.n_wp - 1, wp + v0 * 4, lim + a * 9, tb);
          }
        });
        PolicyRoundIn in{};
        in.n_paths = (int32_t)A;
        in.seg_offsets = so.data();
        in.n_segments = nS;
        in.n_vertices = nV;
        in.block = block;
        in.opt = o.solver;
        if (any_stop && d == 4) in.opt.flags |= MRS_TG_FLAG_CONSTRAINED_SLOTS;
        if (o.max_execution_time_s > 0) in.opt.max_time_s = 2.0 * 0.95 * budget_left;  // :899
        in.max_len_factor = o.max_trajectory_len_factor;
        in.min_len_factor = o.min_trajectory_len_factor;
        in.max_deviation = o.max_deviation;
        in.first_segment = o.max_deviation_first_segment;
        in.check_enabled = o.check_deviation_enabled;
        in.last_round = round == o.max_deviation_iterations;
        in.sample_capacity = sample_capacity;
        in.moving_starts = moving_starts;
        const double t1 = now();
        t_build += t1 - t0;
        const int rc = host.round(in);
        if (rc != MRS_TG_OK) return rc;
        const double t2 = now();
        t_solve += t2 - t1;
        const bool late = overtime();  // findTrajectory's own checks behind optimize() and the sampler: "return {}" (:1085, :1156, :1171)
        const int32_t* r_ok = reinterpret_cast<const int32_t*>(block + L.ok);
        const int32_t* r_ns = reinterpret_cast<const int32_t*>(block + L.ns);
        const double* r_dev = reinterpret_cast<const double*>(block + L.max_dev);
        const uint8_t* r_safe_path = reinterpret_cast<const uint8_t*>(block + L.is_safe);
        const uint8_t* r_safe = reinterpret_cast<const uint8_t*>(block + L.safe);
        const double* r_smp = reinterpret_cast<const double*>(block + L.samples);
        const bool last = in.last_round != 0;
        parallel_ranges(A, 128, [&](size_t a0, size_t a1) {
          std::vector<uint8_t> safe;
          for (size_t a = a0; a < a1; ++a) {
            const int p = active[a];
            const bool ok = !late && r_ok[a] != 0;
            st[p].ok = ok;
            st[p].n_samples = ok ? r_ns[a] : 0;
            if (!ok) {
              st[p].done = true;  // "failed to find trajectory" :720-727, :771-778
              continue;
            }
            bool finished = last;
            if (!last) {
              st[p].max_dev = r_dev[a];
              if (o.check_deviation_enabled && !r_safe_path[a]) {
                safe.assign(r_safe + so[a], r_safe + so[a + 1]);
                insert_midpoints(st[p], safe, o);
                st[p].iterations = round + 1;
              } else {
                st[p].done = true;
                finished = true;
              }
            }
            if (finished)
              std::memcpy(samples_out + (size_t)p * sample_capacity * 4, r_smp + a * (size_t)sample_capacity * 4,
                          sizeof(double) * 4 * (size_t)r_ns[a]);
          }
        });
        t_post += now() - t2;
        if (last) break;
        continue;
      }
    }
    // ---- solve every active path (one batched GPU call, or the fallback sampler on the host)
    if (use_fallback) {
      for (int p : active) {
        double* out = samples_out + (size_t)p * sample_capacity * 4;
        const int ns = fallback_sampling(st[p], limits + (size_t)p * 9, relax_heading && relax_heading[p], o, dt, out, sample_capacity);
        st[p].n_samples = ns;
        st[p].ok = ns <= sample_capacity;
        if (!st[p].ok) st[p].done = true;
      }
    } else {
      // vertices exactly as findTrajectory builds them (:923-977).  The arrays of the round live in ONE block of pinned
      // host memory kept by the context (no allocation, no page faults and no clearing of a 64 KB sample buffer per
      // request and round; the GPU reads and writes pinned arrays in place, and only the sample rows a path has produced
      // travel); the coefficients, which the policy never reads, stay on the device
      const double t0 = now();
      const size_t A = active.size();
      std::vector<int32_t> so(A + 1, 0);
      for (size_t a = 0; a < A; ++a) so[a + 1] = so[a] + st[active[a]].n_wp - 1;
      const size_t nS = (size_t)so.back(), nV = nS + A;
      auto up = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
      const size_t b_wp = up(nV * 4 * sizeof(double)), b_vals = up(nV * 20 * sizeof(double)), b_lim = up(A * 9 * sizeof(double)),
                   b_times = up(nS * sizeof(double)), b_smp = up(A * (size_t)sample_capacity * 4 * sizeof(double)),
                   b_status = up(A * sizeof(int32_t)), b_ns = up(A * sizeof(int32_t)), b_mask = up(nV * 5);
      const size_t need = b_wp + b_vals + b_lim + b_times + b_smp + b_status + b_ns + b_mask;
      char* block = knob::policy_pinned() ? static_cast<char*>(host.scratch(need)) : nullptr;
      std::vector<char> pageable;  // (the runtime refused that much pinned memory: ordinary memory, copied by the runtime)
      if (!block) {
        pageable.resize(need);
        block = pageable.data();
      }
      double* wp = reinterpret_cast<double*>(block);
      double* vals = reinterpret_cast<double*>(block + b_wp);
      double* lim = reinterpret_cast<double*>(block + b_wp + b_vals);
      double* times = reinterpret_cast<double*>(block + b_wp + b_vals + b_lim);
      double* smp = reinterpret_cast<double*>(block + b_wp + b_vals + b_lim + b_times);
      int32_t* status = reinterpret_cast<int32_t*>(block + b_wp + b_vals + b_lim + b_times + b_smp);
      int32_t* ns = reinterpret_cast<int32_t*>(block + b_wp + b_vals + b_lim + b_times + b_smp + b_status);
      uint8_t* mask = reinterpret_cast<uint8_t*>(block + b_wp + b_vals + b_lim + b_times + b_smp + b_status + b_ns);
      parallel_ranges(A, 128, [&](size_t a0, size_t a1) {
        std::vector<double> tb;
        for (size_t a = a0; a < a1; ++a) {
          const int p = active[a];
          const PathState& s = st[p];
          const bool has_init = has_initial_state && has_initial_state[p] && initial_states;
          const size_t v0 = (size_t)so[a] + a;
          std::memset(times + so[a], 0, sizeof(double) * (size_t)(s.n_wp - 1));
          build_vertices(s.wps.data(), s.stop.data(), s.n_wp, has_init ? &initial_states[p] : nullptr, d, wp + v0 * 4, mask + v0 * 5,
                         vals + v0 * 20);
          effective_limits(limits + (size_t)p * 9, relax_heading && relax_heading[p], lim + a * 9);
          st[p].baca_total = baca_total_time(s.n_wp - 1, wp + v0 * 4, lim + a * 9, tb);
        }
      });
      mrs_tg_options so_opt = o.solver;
      so_opt.estimate_times = 1;
      so_opt.sample_capacity = sample_capacity;
      // the length check below is the reference's answer to a runaway (:1178-1199) where its upper side runs; with that side
      // off the product's own runaway rule answers (MRS_TG_STATUS_ROUNDOFF_LIMITED: rejected by code)
      if (o.max_trajectory_len_factor > 0) so_opt.flags |= MRS_TG_FLAG_REFERENCE_STATUS;
      if (o.max_execution_time_s > 0) so_opt.max_time_s = 2.0 * 0.95 * budget_left;  // :899
      const double t1 = now();
      t_build += t1 - t0;
      const int rc = host.solve((int32_t)A, so.data(), wp, mask, vals, lim, &so_opt, times, status, ns, smp);
      if (rc != MRS_TG_OK) return rc;
      const double t2 = now();
      t_solve += t2 - t1;
      const bool late = overtime();  // findTrajectory's own checks behind optimize() and the sampler: "return {}" (:1085, :1156, :1171)
      parallel_ranges(A, 128, [&](size_t a0, size_t a1) {
        for (size_t a = a0; a < a1; ++a) {
          const int p = active[a];
          bool ok = !late && baca::code_accepted(status[a]);  // :1138-1149
          if (ok && baca::length_check(ns[a], dt, st[p].baca_total, o.max_trajectory_len_factor, o.min_trajectory_len_factor) != 0) ok = false;  // :1178-1199
          if (ns[a] > sample_capacity) ok = false;
          st[p].ok = ok;
          st[p].n_samples = ok ? ns[a] : 0;
          if (!ok) {
            st[p].done = true;  // "failed to find trajectory" :720-727, :771-778
          } else {
            std::memcpy(samples_out + (size_t)p * sample_capacity * 4, smp + a * (size_t)sample_capacity * 4,
                        sizeof(double) * 4 * (size_t)ns[a]);
          }
        }
      });
      t_post += now() - t2;
    }
    if (round == o.max_deviation_iterations) break;  // the last re-solve is not validated again (:729)
    // ---- validate, subdivide the unsafe ones
    const double t3 = now();
    parallel_ranges(active.size(), 128, [&](size_t a0, size_t a1) {
      std::vector<uint8_t> safe;
      for (size_t a = a0; a < a1; ++a) {
        const int p = active[a];
        if (st[p].done) continue;
        double md = 0;
        const bool is_safe = validate_spatial(samples_out + (size_t)p * sample_capacity * 4, st[p].n_samples, st[p], o, safe, md);
        st[p].max_dev = md;
        if (o.check_deviation_enabled && !is_safe) {
          insert_midpoints(st[p], safe, o);
          st[p].iterations = round + 1;
        } else {
          st[p].done = true;
        }
      }
    });
    t_validate += now() - t3;
  }
  if (trace)
    std::fprintf(stderr, "mrs_tg_optimize_paths: %d requests, %.3f ms: vertices + estimates %.3f, mrs_tg_solve_batch %.3f, results %.3f, "
                 "validation + mid-points %.3f\n", n_paths, elapsed() * 1e3, t_build * 1e3, t_solve * 1e3, t_post * 1e3, t_validate * 1e3);
  for (int p = 0; p < n_paths; ++p) {
    const PathState& s = st[p];
    success_out[p] = s.ok ? 1 : 0;
    n_samples_out[p] = s.ok ? s.n_samples : 0;
    if (max_deviation_out) max_deviation_out[p] = s.max_dev;
    if (n_waypoints_out) n_waypoints_out[p] = s.n_wp;
    if (iterations_out) iterations_out[p] = s.iterations;
    if (s.ok && o.override_heading_atan2) {  // getTrajectoryReference :1582-1597
      double* smp = samples_out + (size_t)p * sample_capacity * 4;
      for (int it = 0; it + 1 < s.n_samples; ++it) {
        double* a = smp + (size_t)it * 4;
        const double* b = a + 4;
        // the rule is hdg's (mrs_tg_heading.hpp); the distance stays the reference's std::hypot, which hdg::step_xy's written-out
        // square root may miss by an ulp at the threshold
        const double dx = b[0] - a[0], dy = b[1] - a[1];
        if (hdg::is_source(it, std::hypot(dy, dx), hdg::kMinStep)) a[3] = hdg::heading_of(dx, dy);
        else a[3] = smp[(size_t)(it - 1) * 4 + 3];
      }
    }
  }
  return MRS_TG_OK;
}

// getWaypointInTrajectoryIdxs :1461-1499 for one path: returns the number of indices written.  Nothing is read when there
// is no waypoint.
inline int32_t waypoint_trajectory_idxs(const double* samples, int32_t n_samples, const mrs_tg_waypoint* waypoints,
                                        int32_t n_waypoints, int32_t* idxs_out) {
  if (!samples || !waypoints || !idxs_out) return 0;
  int32_t c = 0;
  double miss;
  for (int i = 0; i + 1 < n_samples && c < n_waypoints; ++i)
    if (passq::hit(waypoints[c].coords, samples + (size_t)i * 4, samples + (size_t)(i + 1) * 4, miss)) idxs_out[c++] = i;
  return c;
}

// mrs_tg_default_options: the reference's parameters where it has them
inline void default_solver_options(mrs_tg_options* opt) {
  std::memset(opt, 0, sizeof(*opt));
  opt->derivative_to_optimize = 4;
  opt->time_alloc_method = MRS_TG_TIME_ALLOC_NONE;
  opt->estimate_times = 0;
  opt->max_iterations = 10;  // config/private/trajectory_generation.yaml:10
  opt->f_rel = 0.05;         // src/mrs_trajectory_generation.cpp:884
  opt->f_abs = -1.0;
  opt->x_rel = 0.1;          // src/mrs_trajectory_generation.cpp:885
  opt->x_abs = -1.0;
  opt->sampling_dt = 0.0;
  opt->sample_capacity = 0;
  opt->flags = 0;
  opt->time_penalty = 100.0;           // config/private/trajectory_generation.yaml:4
  opt->soft_constraint_weight = 1.5;   // :6
  opt->use_soft_constraints = 1;       // :5
  opt->initial_stepsize_rel = 0.1;     // src/mrs_trajectory_generation.cpp:893
  opt->max_time_s = 0.0;               // no deadline (the nodelet sets 2 * 0.95 * timeLeft(), :899)
  opt->max_trajectory_len_factor = 3.0;   // config/public/trajectory_generation.yaml:35
  opt->min_trajectory_len_factor = 0.33;  // :36
}

// config/public/trajectory_generation.yaml + config/private/trajectory_generation.yaml; `solver` is filled by the caller
inline void default_policy_fields(mrs_tg_policy_options* o) {
  o->solver.time_alloc_method = MRS_TG_TIME_ALLOC_MELLINGER;  // config/private/trajectory_generation.yaml:7
  o->solver.derivative_to_optimize = 2;                       // :11 (0 -> acceleration)
  o->solver.sampling_dt = 0.2;                                // config/public/trajectory_generation.yaml
  o->check_deviation_enabled = 1;
  o->max_deviation = 0.05;
  o->max_deviation_iterations = 6;
  o->max_deviation_first_segment = 1;
  o->min_waypoint_distance = 0.05;
  o->path_straightener_enabled = 0;
  o->path_straightener_max_deviation = 0.05;
  o->path_straightener_max_hdg_deviation = 0.1;
  o->max_trajectory_len_factor = 3.0;
  o->min_trajectory_len_factor = 0.33;
  o->fallback_sampling = 0;
  o->fallback_speed_factor = 1.0;
  o->fallback_accel_factor = 1.0;
  o->fallback_stopping_time = 2.0;
  o->override_heading_atan2 = 0;
  o->reserved_ = 0;
  o->max_execution_time_s = 0.0;
}

}  // namespace policy
}  // namespace mrs_tg

// mrs_tg_initial.hpp -- where a trajectory starts and what goes in front of it, as the plan steps run it (mrs_tg_initial.hip:
// mrs_tg_plan_initial_condition, mrs_tg_plan_prepend_initial_condition, mrs_tg_plan_splice_prediction and their backward passes);
// DESIGN.md section 11g.  The stages are prepareInitialCondition (mrs_trajectory_generation.cpp:506-614 of the reference), the
// first-waypoint rule with the prepended waypoint (:649-672) and the pre-trajectory of a path stamped in the future (:801-840).
// The public, pure-host statement of the same arithmetic is include/mrs_tg_initial_condition.hpp (mrs_tg::initial_condition);
// this file restates it over plain values for both sides, and tests/host/initial_harness.cpp holds the two to the same answers:
//   sample_offset(offset)  k  = int(ceil((offset * 0.5 - 0.01) / 0.2)) + 1, saturated to the int32 range
//   splice_offset(age)     k2 = int(floor((age - 0.01) / 0.2)) + 1
// in that order of operations.  THE QUOTIENT IS A DIVISION, never a product with a reciprocal: 0.2 is not a power of two, and
// only the correctly rounded quotient puts an offset at a bin edge into the host's bin.
//   decide(...)            the first-case-wins table of initial_condition::prepare -> the decision word (MRS_TG_IC_*) and k
//   splice_plan(...)       what mrs_tg_plan_splice_prediction does with one path: leave it, flag it, report a count that does
//                          not fit, or shift the n rows up by k and put k prediction rows in front
//   chunk walk             the order in which the in-place shift takes its chunks of kSpliceChunk rows: from the last to the
//                          first, every chunk loading all its rows before it stores one, the prefix after the lowest chunk
// Every value the steps produce is a copy of an input, except z + takeoff_height.  Plain double, __host__ __device__, no
// contraction; the only library functions are ceil and floor.
#pragma once

#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace initq {

constexpr double kMpcStep = 0.2;               // the MPC tracker's prediction step (every step but the first)
constexpr double kMpcFirstStep = 0.01;         // its first step (:555)
constexpr double kFirstWaypointFactor = 0.50;  // FUTURIZATION_FIRST_WAYPOINT_FACTOR (:61)
constexpr double kFutureThreshold = 0.2;       // "more than one MPC step ahead" (:552, :652)
constexpr double kTrackerCmdTimeout = 1.0;     // a tracker command older than this is not used (:518)

// the decision word: the values of MRS_TG_IC_* (include/mrs_tg.h; mrs_tg_initial.hip asserts that they are the same)
constexpr int32_t kPrepend = 1, kFromFuture = 2, kDropFirst = 4, kFromTracker = 8, kFromUav = 16, kFromPrediction = 32,
                  kInvalid = 64;
// flags_dev of mrs_tg_plan_initial_condition
constexpr int32_t kHaveTracker = 1, kHaveUav = 2, kDontPrepend = 4;

constexpr int kSpliceChunk = 64;  // rows the in-place shift loads before it stores any: one wavefront's lanes

MRS_TG_HD inline bool is_nan(double v) { return v != v; }

// int(q) + 1 for an integral double q, clamped to the int32 range (a NaN gives the upper end)
MRS_TG_HD inline int32_t saturated_plus_one(double q) {
  if (!(q < 2147483647.0)) return 2147483647;
  if (!(q > -2147483649.0)) return -2147483647 - 1;
  return static_cast<int32_t>(static_cast<int64_t>(q) + 1);
}

// path_sample_offset of :557: the prediction sample the initial condition is taken from
MRS_TG_HD inline int32_t sample_offset(double path_time_offset_s) {
  MRS_TG_NO_CONTRACT
  const double half = path_time_offset_s * kFirstWaypointFactor;
  const double shifted = half - kMpcFirstStep;
  const double steps = shifted / kMpcStep;
  return saturated_plus_one(ceil(steps));
}

// path_sample_offset_2 of :805-806: the prediction sample that is "now" when the trajectory is ready
MRS_TG_HD inline int32_t splice_offset(double prediction_age_s) {
  MRS_TG_NO_CONTRACT
  const double shifted = prediction_age_s - kMpcFirstStep;
  const double steps = shifted / kMpcStep;
  return saturated_plus_one(floor(steps));
}

struct Decision {
  int32_t word;  // MRS_TG_IC_* bits
  int32_t k;     // path_sample_offset as prepareInitialCondition returns it: set when the tracker command is used for a path
                 // from the future, whether the prediction reaches that far or not; else 0
};

// initial_condition::prepare over plain values; the first case that holds decides.  kInvalid stands alone: a NaN offset, a NaN
// age of a tracker command that is present, an n_pred outside [0, pred_capacity].
MRS_TG_HD inline Decision decide(bool have_tracker, double tracker_age_s, bool have_uav, bool dont_prepend,
                                 double path_time_offset_s, int32_t n_path_waypoints, int32_t n_pred, int32_t pred_capacity) {
  Decision d;
  d.word = 0, d.k = 0;
  if (is_nan(path_time_offset_s) || (have_tracker && is_nan(tracker_age_s)) || n_pred < 0 || n_pred > pred_capacity) {
    d.word = kInvalid;
    return d;
  }
  const bool future = path_time_offset_s > kFutureThreshold;
  if (future && n_path_waypoints >= 2) d.word |= kDropFirst;  // before prepareInitialCondition, whatever it decides
  if (dont_prepend) return d;
  if (!have_tracker || tracker_age_s > kTrackerCmdTimeout) {  // before takeoff (:518-537)
    if (have_uav) d.word |= kPrepend | kFromUav;
    return d;
  }
  d.word |= kPrepend;
  if (future) {
    d.k = sample_offset(path_time_offset_s);
    if (d.k <= n_pred - 1) {  // else "can not extrapolate into the waypoints, using tracker_cmd instead" (:559-562)
      d.word |= kFromFuture | kFromPrediction;
      return d;
    }
  }
  d.word |= kFromTracker;
  return d;
}

// ---- the splice -----------------------------------------------------------------------------------------------------------------

enum SpliceAction : int32_t {
  kLeave = 0,     // dead, overflowed by the sampler, or no splice needed: rows and count stay
  kShort = 1,     // the prediction has fewer than k rows (or its age is NaN): flagged, rows and count stay
  kTooLong = 2,   // n + k rows do not fit the capacity: only the count n + k is reported
  kInsert = 3     // rows 0 .. n-1 move to k .. n+k-1, prediction rows 0 .. k-1 go in front
};
struct SplicePlan {
  int32_t action;
  int32_t n;      // the rows the path has (0 .. capacity) where the action is kTooLong or kInsert
  int32_t k;      // the rows that go in front
  int32_t count;  // the count to report where the action is kTooLong or kInsert: n + k, saturated to the int32 range
};

// n_samples as the sampler left it, n_pred already cut to [0, pred_capacity] by the caller
MRS_TG_HD inline SplicePlan splice_plan(bool live, int32_t n_samples, int32_t capacity, int32_t decision, int32_t k,
                                        double prediction_age_s, int32_t n_pred) {
  SplicePlan s;
  s.action = kLeave, s.n = 0, s.k = 0, s.count = 0;
  if (!live || n_samples < 0 || n_samples > capacity) return s;  // (capacity + 1: the sampler ran over)
  if ((decision & kFromFuture) == 0 || (decision & kInvalid) != 0 || k <= 0) return s;
  if (is_nan(prediction_age_s)) {
    s.action = kShort;
    return s;
  }
  if (k <= splice_offset(prediction_age_s)) return s;
  if (k > n_pred) {
    s.action = kShort;
    return s;
  }
  const int64_t need = static_cast<int64_t>(n_samples) + k;
  s.n = n_samples, s.k = k;
  s.count = need > 2147483647ll ? 2147483647 : static_cast<int32_t>(need);
  s.action = need > capacity ? kTooLong : kInsert;
  return s;
}

// The in-place shift's walk: chunk c holds the rows c * kSpliceChunk .. ; the chunks are taken from splice_chunks(n) - 1 down
// to 0.  Chunk c's stores land at or behind row c * kSpliceChunk + k, behind everything the chunks below still have to load,
// and the prefix's rows 0 .. k-1 are stored when every row has been loaded: correct for every k > 0.
MRS_TG_HD inline int32_t splice_chunks(int32_t n) { return (n + kSpliceChunk - 1) / kSpliceChunk; }

// ---- backward -------------------------------------------------------------------------------------------------------------------

// which row of a prediction array takes the gradient of the initial condition: k where the decision took the prediction and k
// lies inside the array, else none (-1)
MRS_TG_HD inline int32_t prediction_row(int32_t decision, int32_t k, int32_t pred_capacity) {
  return (decision & kFromPrediction) != 0 && k >= 0 && k < pred_capacity ? k : -1;
}

// the edit of :649-672 for one path with nv requested vertices: how many go (0 or 1), whether one comes in front, what is left
struct Prepend {
  int32_t drop, prepend, count;
};
MRS_TG_HD inline Prepend prepend_plan(int32_t decision, int32_t nv) {
  Prepend e;
  nv = nv < 0 ? 0 : nv;
  e.drop = (decision & kDropFirst) != 0 && (decision & kInvalid) == 0 && nv >= 1 ? 1 : 0;
  e.prepend = (decision & kPrepend) != 0 && (decision & kInvalid) == 0 ? 1 : 0;
  e.count = nv - e.drop + e.prepend;
  return e;
}

}  // namespace initq
}  // namespace mrs_tg

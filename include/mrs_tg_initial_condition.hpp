// mrs_tg_initial_condition.hpp -- the initial condition of a request, including paths stamped in the future: the PURE-HOST
// arithmetic of MrsTrajectoryGeneration::prepareInitialCondition (the reference's src/mrs_trajectory_generation.cpp:506-614),
// the first-waypoint rule of optimize() (:650-655) and the splice of the MPC prediction in front of a trajectory from the
// future (:801-838).  O(1) per request plus at most one prediction's rows copied; no HIP type or call appears here.
// Header-only and public: mrs_tg_abi.hip exports it as mrs_tg_prepare_initial_condition / mrs_tg_splice_prediction,
// mrs_tg_service.hpp uses it inline, and it compiles with plain g++ (tests/host/initial_condition_harness.cpp runs it under
// ASan / UBSan).
//
// Every time is in seconds and already a difference: the caller reads its clock and passes "path stamp - now", "now - tracker
// command stamp" and "now - prediction stamp".  The prediction is mrs_msgs::MpcPredictionFullState already transformed into the
// path's frame (the tf stays on the ROS side).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "mrs_tg.h"

namespace mrs_tg {
namespace initial_condition {

constexpr double kMpcStep = 0.2;                // the MPC tracker's prediction step (every step but the first)
constexpr double kMpcFirstStep = 0.01;          // its first step: "0.01 is subtracted for the first sample" (:555)
constexpr double kFirstWaypointFactor = 0.50;   // FUTURIZATION_FIRST_WAYPOINT_FACTOR (:61)
constexpr double kFutureThreshold = 0.2;        // "more than one MPC step ahead" (:552, :652)
constexpr double kTrackerCmdTimeout = 1.0;      // a tracker command older than this is not used (:518)
constexpr double kFutureSamplingDt = 0.2;       // sampling_dt of a path from the future (:692-697)

// int(q) + 1 for an integral double q, clamped to the int32 range instead of the undefined conversion of an out-of-range double
inline int32_t saturated_plus_one(double q) {
  if (!(q < 2147483647.0)) return INT32_MAX;   // q + 1 > INT32_MAX (and NaN)
  if (!(q > -2147483649.0)) return INT32_MIN;  // q + 1 < INT32_MIN
  return static_cast<int32_t>(static_cast<int64_t>(q) + 1);
}

// path_sample_offset of :557: the prediction sample the initial condition is taken from, for an offset > 0.2 s.  Evaluated in
// double in the reference's order -- the products and quotients decide the bins exactly (offset * 0.5 is exact).
inline int32_t sample_offset(double path_time_offset_s) {
  const double half = path_time_offset_s * kFirstWaypointFactor;
  const double shifted = half - kMpcFirstStep;
  const double steps = shifted / kMpcStep;
  return saturated_plus_one(std::ceil(steps));
}

// path_sample_offset_2 of :805-806: the prediction sample that is "now" when the trajectory is ready, age = now - prediction stamp
inline int32_t splice_offset(double prediction_age_s) {
  const double shifted = prediction_age_s - kMpcFirstStep;
  const double steps = shifted / kMpcStep;
  return saturated_plus_one(std::floor(steps));
}

struct Decision {
  bool has_initial_condition = false;  // a waypoint is prepended and initial_state is the solve's initial condition
  bool from_future = false;            // sample at kFutureSamplingDt and splice the prediction afterwards
  bool drop_first_waypoint = false;    // erase the path's first waypoint before prepending (:650-655)
  int32_t sample_offset = 0;           // path_sample_offset as prepareInitialCondition returns it
  mrs_tg_waypoint waypoint{};          // the initial condition as a waypoint (stop_at = 0)
  mrs_tg_initial_state state{};        // ... and its derivatives
};

inline int refuse(const char** error, const char* why) {
  *error = why;
  return MRS_TG_ERR_INVALID_ARG;
}

inline bool prediction_valid(const mrs_tg_prediction* p) {
  return p == nullptr || p->n_samples == 0 ||
         (p->n_samples > 0 && p->position && p->velocity && p->acceleration && p->jerk);
}

// prepareInitialCondition (:506-614) preceded by the first-waypoint rule (:650-655), for one request.
//   tracker_pose / tracker_state: the tracker command (position + heading / heading and derivatives), both NULL when there is none;
//   tracker_age_s: now - its stamp; prediction: its full_state_prediction (NULL or 0 samples: none);
//   uav_pose4: x, y, z, heading of the UAV state, NULL when there is none; path_time_offset_s: path stamp - now, 0 for an
//   unstamped path.  Returns MRS_TG_OK, or MRS_TG_ERR_INVALID_ARG with *error set (then *out is untouched).
inline int prepare(const mrs_tg_waypoint* tracker_pose, const mrs_tg_initial_state* tracker_state, double tracker_age_s,
                   const mrs_tg_prediction* prediction, const double* uav_pose4, double takeoff_height, double path_time_offset_s,
                   int32_t n_path_waypoints, bool dont_prepend, Decision* out, const char** error) {
  const bool have_tracker = tracker_pose != nullptr;
  if (!out) return refuse(error, "no output");
  if (have_tracker != (tracker_state != nullptr)) return refuse(error, "tracker_pose and tracker_state go together");
  if (n_path_waypoints < 0) return refuse(error, "n_path_waypoints < 0");
  if (std::isnan(path_time_offset_s)) return refuse(error, "the path's time offset is NaN");
  if (have_tracker && std::isnan(tracker_age_s)) return refuse(error, "the tracker command's age is NaN");
  if (!prediction_valid(prediction)) return refuse(error, "a prediction with samples needs all four arrays");
  if (uav_pose4 && std::isnan(takeoff_height)) return refuse(error, "takeoff_height is NaN");

  Decision d;
  const bool future = path_time_offset_s > kFutureThreshold;
  d.drop_first_waypoint = future && n_path_waypoints >= 2;  // before prepareInitialCondition, whatever it decides
  if (dont_prepend) {
    *out = d;
    return MRS_TG_OK;
  }
  if (!have_tracker || tracker_age_s > kTrackerCmdTimeout) {  // before takeoff: the UAV state lifted by the takeoff height (:518-537)
    if (uav_pose4) {
      d.has_initial_condition = true;
      d.waypoint.coords[0] = uav_pose4[0];
      d.waypoint.coords[1] = uav_pose4[1];
      d.waypoint.coords[2] = uav_pose4[2] + takeoff_height;
      d.waypoint.coords[3] = uav_pose4[3];
      d.state.heading = uav_pose4[3];
    }
    *out = d;
    return MRS_TG_OK;
  }
  d.has_initial_condition = true;
  d.waypoint = *tracker_pose;
  d.waypoint.stop_at = 0;
  d.state = *tracker_state;
  if (future) {
    d.sample_offset = sample_offset(path_time_offset_s);
    const int32_t n_pred = prediction ? prediction->n_samples : 0;
    if (d.sample_offset <= n_pred - 1) {  // else "can not extrapolate into the waypoints, using tracker_cmd instead" (:559-562)
      const size_t row = 4 * static_cast<size_t>(d.sample_offset);
      std::memcpy(d.waypoint.coords, prediction->position + row, 4 * sizeof(double));
      d.state.heading = prediction->position[row + 3];
      std::memcpy(d.state.velocity, prediction->velocity + row, 4 * sizeof(double));
      std::memcpy(d.state.acceleration, prediction->acceleration + row, 4 * sizeof(double));
      std::memcpy(d.state.jerk, prediction->jerk + row, 4 * sizeof(double));
      d.from_future = true;
    }
  }
  *out = d;
  return MRS_TG_OK;
}

// The pre-trajectory of :801-838: when sample_offset > splice_offset(prediction_age_s), prediction rows 0 .. sample_offset-1
// (position + heading) go in front of samples [n_samples][4], in that order.  Returns the spliced count (n_samples when nothing
// is inserted) and writes only if it fits sample_capacity; a negative MRS_TG_ERR_* with *error set for invalid arguments,
// among them a prediction with fewer than sample_offset rows.
inline int32_t splice(const mrs_tg_prediction* prediction, int32_t sample_offset, double prediction_age_s, double* samples,
                      int32_t n_samples, int32_t sample_capacity, const char** error) {
  if (n_samples < 0 || sample_capacity < 0) return refuse(error, "negative sample count or capacity");
  if (n_samples > 0 && !samples) return refuse(error, "samples is NULL");
  if (std::isnan(prediction_age_s)) return refuse(error, "the prediction's age is NaN");
  if (!prediction_valid(prediction)) return refuse(error, "a prediction with samples needs all four arrays");
  if (sample_offset <= splice_offset(prediction_age_s) || sample_offset <= 0) return n_samples;  // nothing to insert
  const int32_t n_pred = prediction ? prediction->n_samples : 0;
  if (sample_offset > n_pred) return refuse(error, "the prediction has fewer samples than the sample offset");
  const int64_t need = static_cast<int64_t>(n_samples) + sample_offset;
  if (need > INT32_MAX) return refuse(error, "the spliced trajectory exceeds the int32 range");
  if (need > sample_capacity) return static_cast<int32_t>(need);
  if (n_samples > 0) std::memmove(samples + 4 * static_cast<size_t>(sample_offset), samples, 4 * sizeof(double) * n_samples);
  std::memcpy(samples, prediction->position, 4 * sizeof(double) * static_cast<size_t>(sample_offset));
  return static_cast<int32_t>(need);
}

}  // namespace initial_condition
}  // namespace mrs_tg

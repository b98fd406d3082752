// future_path_host.cpp -- the initial condition of include/mrs_tg_service.hpp on a fixed clock: a request before takeoff, a
// path stamped in the future (MPC prediction sample as the start, first waypoint dropped, 0.2 s sampling, the prediction's
// first samples spliced in front), a stamp beyond the prediction's horizon, a stale tracker command, a batch that mixes
// future and present requests, and a service that never sees any of the new inputs.  Prints one JSON object (the samples with
// 17 significant digits, so that the reader can compare bits); tests/test_gpu_future_paths.py builds it with g++ against
// libmrs_tg.so and checks it.
//
//   g++ -std=c++17 -I include examples/future_path_host.cpp -o future_path_host
//     -L mrs_uav_trajectory_generation_amd -lmrs_tg -Wl,-rpath,$PWD/mrs_uav_trajectory_generation_amd
#include <cstdio>
#include <vector>

#include "mrs_tg_service.hpp"

using namespace mrs_tg;

static const double kNow = 1000.0;  // the service's clock stands still: every offset below is exact

static Constraints constraints() {  // the reference tests' limits (as examples/path_service_host.cpp)
  Constraints c;
  c.horizontal_speed = 2.0;
  c.horizontal_acceleration = 2.0;
  c.horizontal_jerk = 20.0;
  c.vertical_ascending_speed = 2.0;
  c.vertical_descending_speed = 2.0;
  c.vertical_ascending_acceleration = 2.0;
  c.vertical_descending_acceleration = 2.0;
  c.vertical_ascending_jerk = 20.0;
  c.vertical_descending_jerk = 20.0;
  c.heading_speed = 1.0;
  c.heading_acceleration = 2.0;
  c.heading_jerk = 20.0;
  return c;
}

static Path test_path() {  // test/get_path_before_takeoff/test.cpp:29-32
  Path p;
  p.frame_id = "uav1/world_origin";
  p.use_heading = true;
  p.fly_now = true;
  p.points = {{-5, -5, 5, 1}, {-5, 5, 5, 2}, {5, -5, 5, 3}, {5, 5, 5, 4}};
  return p;
}

// a planner's continuation of the flight: the UAV flies along +x at 1 m/s, z = 3, and the path goes on from where it will be
static Path straight_path(double stamp) {
  Path p;
  p.frame_id = "uav1/world_origin";
  p.use_heading = true;
  p.fly_now = true;
  p.stamp = stamp;
  p.points = {{2, 0, 3, 0}, {6, 0, 3, 0}, {10, 0, 3, 0}, {10, 4, 3, 0}};
  return p;
}

static CurrentState tracker(double stamp) {
  CurrentState s;
  s.position = {0.0, 0.0, 3.0, 0.0};
  s.velocity = {1.0, 0.0, 0.0, 0.0};
  s.stamp = stamp;
  return s;
}

// the MPC prediction of that flight: sample 0 now, then 0.01 s, then 0.2 s steps; 41 samples
static Prediction prediction(double stamp) {
  Prediction p;
  p.stamp = stamp;
  for (int i = 0; i < 41; ++i) {
    const double t = i == 0 ? 0.0 : 0.01 + 0.2 * (i - 1);
    p.position.push_back({t, 0.0, 3.0, 0.0});
    p.velocity.push_back({1.0, 0.0, 0.0, 0.0});
    p.acceleration.push_back({0.0, 0.0, 0.0, 0.0});
    p.jerk.push_back({0.0, 0.0, 0.0, 0.0});
  }
  return p;
}

static ServiceParams params(double sampling_dt) {
  ServiceParams sp;
  sp.max_time = 0;  // no deadline: what is solved does not depend on how fast the machine is
  sp.takeoff_height = 1.5;
  sp.policy.solver.sampling_dt = sampling_dt;
  return sp;
}

static bool same(const GetPathResponse& a, const GetPathResponse& b) {
  if (a.success != b.success || a.message != b.message || a.trajectory.dt != b.trajectory.dt ||
      a.trajectory.fly_now != b.trajectory.fly_now || a.waypoint_trajectory_idxs != b.waypoint_trajectory_idxs ||
      a.max_deviation != b.max_deviation || a.trajectory.points.size() != b.trajectory.points.size())
    return false;
  for (size_t i = 0; i < a.trajectory.points.size(); ++i) {
    const Reference &p = a.trajectory.points[i], &q = b.trajectory.points[i];
    if (p.x != q.x || p.y != q.y || p.z != q.z || p.heading != q.heading) return false;
  }
  return true;
}

static void print_response(const char* name, const GetPathResponse& r) {
  printf("\"%s\": {\"success\": %s, \"message\": \"%s\", \"dt\": %.17g, \"fly_now\": %s, \"max_deviation\": %.17g, \"idxs\": [", name,
         r.success ? "true" : "false", r.message.c_str(), r.trajectory.dt, r.trajectory.fly_now ? "true" : "false", r.max_deviation);
  for (size_t i = 0; i < r.waypoint_trajectory_idxs.size(); ++i) printf("%s%d", i ? ", " : "", r.waypoint_trajectory_idxs[i]);
  printf("], \"points\": [");
  for (size_t i = 0; i < r.trajectory.points.size(); ++i) {
    const Reference& q = r.trajectory.points[i];
    printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", q.x, q.y, q.z, q.heading);
  }
  printf("]},\n");
}

int main() {
  printf("{\n");
  {  // 1. before takeoff: no tracker command, the UAV on the ground -> the start is the UAV state + takeoff height
    PathService srv(0, params(0.2));
    srv.setClock([] { return kNow; });
    srv.setConstraints(constraints());
    srv.setUavState({0.0, 0.0, 0.0, 0.5});
    print_response("before_takeoff", srv.getPath(test_path()));
  }
  {
    PathService srv(0, params(0.1));  // sampling_dt 0.1: a path from the future is sampled at 0.2 s all the same
    srv.setClock([] { return kNow; });
    srv.setConstraints(constraints());
    srv.setCurrentState(tracker(kNow - 0.05));
    srv.setPrediction(prediction(kNow - 0.05));
    srv.setUavState({0.0, 0.0, 3.0, 0.0});
    // 2. stamped 2.0 s ahead: k = 6, the prediction 0.05 s old (k2 = 1) -> rows 0..5 in front
    const Path future = straight_path(kNow + 2.0);
    const GetPathResponse f = srv.getPath(future);
    print_response("future", f);
    // 3. stamped 20 s ahead: k = 51 lies beyond the 41 samples -> the tracker command, sampling_dt, no prefix; the first
    //    waypoint (off the line) is dropped all the same
    Path beyond = straight_path(kNow + 20.0);
    beyond.points[0] = {-3, 5, 3, 0};
    const GetPathResponse b = srv.getPath(beyond);
    print_response("beyond_horizon", b);
    // 5. a batch mixing future and present requests: each answer is the answer to that request alone
    Path present = straight_path(0.0);
    const GetPathResponse p = srv.getPath(present);
    print_response("present", p);
    const auto mixed = srv.getPaths({present, future, beyond, future, present});
    const bool equal = same(mixed[0], p) && same(mixed[1], f) && same(mixed[2], b) && same(mixed[3], f) && same(mixed[4], p);
    printf("\"mixed_equals_alone\": %s,\n", equal ? "true" : "false");
    // 4. the tracker command 1.5 s old: stale -> the UAV state + takeoff height, even for a stamped path
    srv.setCurrentState(tracker(kNow - 1.5));
    print_response("stale_tracker", srv.getPath(test_path()));
    print_response("stale_tracker_future", srv.getPath(future));
  }
  {  // 6. none of the new inputs: the service as it was used before they existed
    PathService srv(0, params(0.2));
    srv.setConstraints(constraints());
    CurrentState s;
    s.position = {0.0, 0.0, 3.0, 0.5};
    srv.setCurrentState(s);
    Path loop = test_path();
    loop.loop = true;
    loop.stop_at_waypoints = true;
    Path fast = test_path();  // a user override of the limits, tested against the current state (:997-1026)
    fast.override_constraints = true;
    fast.override_max_velocity_horizontal = 4.0;
    fast.override_max_velocity_vertical = 2.0;
    fast.override_max_acceleration_horizontal = 3.0;
    fast.override_max_acceleration_vertical = 2.0;
    fast.override_max_jerk_horizontal = 30.0;
    fast.override_max_jerk_vertical = 30.0;
    const std::vector<Path> paths = {test_path(), loop, fast, Path()};
    const auto r = srv.getPaths(paths);
    print_response("untouched_plain", r[0]);
    print_response("untouched_loop", r[1]);
    print_response("untouched_override", r[2]);
    print_response("untouched_empty", r[3]);
    // 7. the new inputs set where they do not apply: unstamped paths, a tracker command stamped 0.1 s ago, a prediction and a
    //    UAV state -> the same answers, bit for bit
    PathService srv2(0, params(0.2));
    srv2.setClock([] { return kNow; });
    srv2.setConstraints(constraints());
    s.stamp = kNow - 0.1;
    srv2.setCurrentState(s);
    srv2.setPrediction(prediction(kNow - 0.05));
    srv2.setUavState({5.0, 5.0, 0.0, 0.0});
    const auto r2 = srv2.getPaths(paths);
    bool equal = r2.size() == r.size();
    for (size_t i = 0; equal && i < r.size(); ++i) equal = same(r[i], r2[i]);
    printf("\"inputs_that_do_not_apply_change_nothing\": %s,\n", equal ? "true" : "false");
  }
  printf("\"done\": true\n}\n");
  return 0;
}

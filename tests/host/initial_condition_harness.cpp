// initial_condition_harness.cpp -- include/mrs_tg_initial_condition.hpp (the host arithmetic
// behind mrs_tg_prepare_initial_condition / mrs_tg_splice_prediction) compiled with plain g++, for the sanitizers
// (tests/test_initial_condition_sanitizers.py).  Every array it hands over is a heap block of exactly the size the call may
// touch, so a read or write past one is an AddressSanitizer report.  Prints one line per case; the test compares the lines
// with its numpy restatement of the reference.
//
//   g++ -std=c++17 -fsanitize=address,undefined tests/host/initial_condition_harness.cpp -o harness && ./harness
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/mrs_tg_initial_condition.hpp"

namespace ic = mrs_tg::initial_condition;

struct HeapPrediction {  // four exact-size heap blocks; row i, column c of array a holds 100 a + i + c / 8
  double* rows[4] = {nullptr, nullptr, nullptr, nullptr};
  mrs_tg_prediction view{};
  explicit HeapPrediction(int n) {
    view.n_samples = n;
    for (int a = 0; a < 4 && n > 0; ++a) {
      rows[a] = static_cast<double*>(std::malloc(sizeof(double) * 4 * n));
      for (int i = 0; i < n; ++i)
        for (int c = 0; c < 4; ++c) rows[a][4 * i + c] = 100.0 * a + i + c / 8.0;
    }
    view.position = rows[0];
    view.velocity = rows[1];
    view.acceleration = rows[2];
    view.jerk = rows[3];
  }
  ~HeapPrediction() {
    for (double* r : rows) std::free(r);
  }
};

static void print_doubles(const double* v, int n) {
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double ages[] = {-1.0, 1.0, std::nextafter(1.0, 2.0), 0.3};  // first entry: no tracker command
  const double offsets[] = {0.0, 0.2, std::nextafter(0.2, 1.0), 2.0, 20.0, 1e300, inf, -3.0, nan};
  const int pred_sizes[] = {0, 41};
  int cases = 0, errors = 0;

  mrs_tg_waypoint* pose = static_cast<mrs_tg_waypoint*>(std::malloc(sizeof(mrs_tg_waypoint)));
  mrs_tg_initial_state* state = static_cast<mrs_tg_initial_state*>(std::malloc(sizeof(mrs_tg_initial_state)));
  double* uav = static_cast<double*>(std::malloc(4 * sizeof(double)));
  *pose = mrs_tg_waypoint{{1.0, -2.0, 3.5, 0.7}, 1};
  *state = mrs_tg_initial_state{0.7, {0.4, -0.2, 0.1, 0.05}, {0.1, 0.2, -0.3, 0.01}, {1.0, -1.0, 0.5, 0.2}};
  uav[0] = 0.25, uav[1] = -0.5, uav[2] = 0.0, uav[3] = -1.2;

  // prepareInitialCondition + the first-waypoint rule: tracker x offset x prediction x dont_prepend x waypoints x UAV state
  for (int t = 0; t < 4; ++t)
    for (double off : offsets)
      for (int np : pred_sizes)
        for (int dont = 0; dont < 2; ++dont)
          for (int n_wp = 1; n_wp <= 2; ++n_wp)
            for (int u = 0; u < 2; ++u) {
              HeapPrediction pred(np);
              ic::Decision d;
              const char* why = "";
              const bool tracker = t > 0;
              const int rc = ic::prepare(tracker ? pose : nullptr, tracker ? state : nullptr, ages[t], &pred.view, u ? uav : nullptr, 1.5,
                                         off, n_wp, dont != 0, &d, &why);
              ++cases;
              std::printf("P %d %.17g %d %d %d %d rc %d", t, off, np, dont, n_wp, u, rc);
              if (rc == MRS_TG_OK) {
                std::printf(" %d %d %d %d", (int)d.has_initial_condition, (int)d.from_future, d.sample_offset, (int)d.drop_first_waypoint);
                print_doubles(d.waypoint.coords, 4);
                std::printf(" %.17g", d.state.heading);
                print_doubles(d.state.velocity, 4);
                print_doubles(d.state.acceleration, 4);
                print_doubles(d.state.jerk, 4);
              } else {
                ++errors;
              }
              std::printf("\n");
            }

  // the splice: sample offsets around the horizon, prediction ages around the bins of k2, buffers of exactly the capacity
  const int ks[] = {0, 1, 2, 6, 40, 41, 42};
  const double splice_ages[] = {-1e300, -0.5, 0.0, 0.01, std::nextafter(0.01, 1.0), 0.21, 1.0, 8.0, nan};
  HeapPrediction pred(41);
  for (int k : ks)
    for (double age : splice_ages)
      for (int n = 0; n <= 5; n += 5)
        for (int extra = -1; extra <= 0; ++extra) {
          const int cap = n + k + extra < n ? n : n + k + extra;
          double* buf = static_cast<double*>(std::malloc(sizeof(double) * 4 * (cap > 0 ? cap : 1)));
          for (int i = 0; i < 4 * cap; ++i) buf[i] = -1000.0 - i;
          const char* why = "";
          const int32_t m = ic::splice(&pred.view, k, age, buf, n, cap, &why);
          ++cases;
          std::printf("S %d %.17g %d %d ret %d", k, age, n, cap, m);
          if (m >= 0) print_doubles(buf, 4 * cap);
          else ++errors;
          std::printf("\n");
          std::free(buf);
        }
  // without a prediction, and with one that is shorter than k: an error, nothing read
  {
    HeapPrediction none(0), short3(3);
    double* buf = static_cast<double*>(std::malloc(sizeof(double) * 4 * 8));
    const char* why = "";
    const int32_t a = ic::splice(&none.view, 4, 0.0, buf, 0, 8, &why);
    const int32_t b = ic::splice(&short3.view, 4, 0.0, buf, 0, 8, &why);
    const int32_t c = ic::splice(nullptr, 4, 0.0, buf, 0, 8, &why);
    cases += 3;
    std::printf("E %d %d %d\n", a, b, c);
    std::free(buf);
  }
  std::free(pose);
  std::free(state);
  std::free(uav);
  std::printf("OK %d cases, %d refused\n", cases, errors);
  return 0;
}

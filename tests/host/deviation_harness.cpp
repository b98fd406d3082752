// deviation_harness.cpp -- the deviation of sampled trajectories from their waypoint polyline and its backward pass
// (csrc/mrs_tg_deviation.hpp: the distance, the advance test and the gradient rows path_deviation_kernel /
// path_deviation_vjp_kernel run) compiled with plain g++ for the CPU, with the scan written as the reference writes it -- one
// sample after the other -- and the sums in the order the header states.  tests/test_deviation_host.py checks it against the
// oracle bit for bit and against 60-digit fixtures; tests/test_gpu_deviation.py checks the kernels against it bit for bit.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/deviation_harness.cpp -o deviation_harness && ./deviation_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   S n_samples capacity first_segment status, waypoints [S + 1][3], samples [m][3] with m = min(n_samples, capacity),
//   upstream [max(m - 1, 0)]
// Output per path, one line: per scanned sample its cursor and its deviation; the maximum and its index; the segment
// maxima [S]; dL/dsamples [max(m - 1, 0)][3]; dL/dwaypoints [S + 1][3]; then what devq::validate -- the scan of the policy
// layer's host route and of policy_validate_kernel -- returns for max_deviation 0.05 and 0.2: is_safe, safe [S], the maximum.
// status <= 0: nothing is scanned.  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_deviation.hpp"

namespace dq = mrs_tg::devq;

int main() {
  for (;;) {
    int S = 0, n = 0, cap = 0, first = 0, status = 0;
    if (std::scanf("%d", &S) != 1) return 0;
    if (std::scanf("%d %d %d %d", &n, &cap, &first, &status) != 4) return 2;
    if (S < 1 || cap < 0) return 2;
    int m = n < cap ? n : cap;
    m = m < 0 ? 0 : m;
    const int k = m > 1 ? m - 1 : 0;
    std::vector<double> w((size_t)(S + 1) * 3), s((size_t)m * 3), g(k);
    for (std::vector<double>* v : {&w, &s, &g})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    const int scanned = status > 0 ? k : 0;
    std::vector<double> seg_max(S, 0.0), gs((size_t)k * 3, 0.0), gw((size_t)(S + 1) * 3, 0.0);
    double max_dev = 0.0;
    int arg = -1, c = 0;
    for (int i = 0; i < scanned; ++i) {
      const double* p = s.data() + (size_t)i * 3;
      const double* a = w.data() + (size_t)c * 3;
      const double d = dq::dist(p, a, a + 3);
      std::printf("%d %.17g ", c, d);
      if (dq::counted(c, first, S)) {
        if (d > max_dev) max_dev = d, arg = i;
        if (d > seg_max[c]) seg_max[c] = d;
      }
      double gp[3], ga[3], gb[3];
      dq::dist_vjp(p, a, a + 3, g[i], gp, ga, gb);
      for (int j = 0; j < 3; ++j) {
        gs[(size_t)i * 3 + j] = gp[j];
        gw[(size_t)c * 3 + j] = dq::accumulate(gw[(size_t)c * 3 + j], ga[j]);
        gw[(size_t)(c + 1) * 3 + j] = dq::accumulate(gw[(size_t)(c + 1) * 3 + j], gb[j]);
      }
      if (dq::advances(a + 3, p, p + 3, c, S)) ++c;
    }
    std::printf("%.17g %d ", max_dev, arg);
    for (double x : seg_max) std::printf("%.17g ", x);
    for (double x : gs) std::printf("%.17g ", x);
    for (double x : gw) std::printf("%.17g ", x);
    std::vector<double> w4((size_t)(S + 1) * 4, 0.0), s4((size_t)m * 4, 0.0);  // (validate reads rows of four)
    for (size_t e = 0; e < w.size(); ++e) w4[e / 3 * 4 + e % 3] = w[e];
    for (size_t e = 0; e < s.size(); ++e) s4[e / 3 * 4 + e % 3] = s[e];
    for (double threshold : {0.05, 0.2}) {
      std::vector<uint8_t> safe(S, 0);
      const dq::Validation v = dq::validate(s4.data(), status > 0 ? m : 0, w4.data(), S + 1, first, threshold, safe.data());
      std::printf("%d ", v.is_safe ? 1 : 0);
      for (uint8_t f : safe) std::printf("%d ", (int)f);
      std::printf("%.17g ", v.max_deviation);
    }
    std::printf("\n");
  }
}

// heading_harness.cpp -- the heading along the direction of travel and its backward pass (csrc/mrs_tg_heading.hpp: the step,
// the source test, the heading and the gradient rows travel_heading_kernel / travel_heading_vjp_kernel run) compiled with plain
// g++ for the CPU, with the stage written as the reference writes it -- one row after the other, a slow row taking the heading
// of the row in front -- and the sums in the order the header states.  tests/test_heading_host.py checks it against the numpy
// and torch restatements of tests/heading_util.py; tests/test_gpu_heading.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/heading_harness.cpp -o heading_harness && ./heading_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   n_samples capacity status min_step, samples [m][4] with m = min(n_samples, capacity), upstream [m][4]
// Output per path, one line: m (0 for status <= 0), per row its source (-1 for the last row) and its heading, then dL/dsamples
// [m][4].  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_heading.hpp"

namespace hq = mrs_tg::hdg;

int main() {
  for (;;) {
    int n = 0, cap = 0, status = 0;
    double min_step = 0.0;
    if (std::scanf("%d", &n) != 1) return 0;
    if (std::scanf("%d %d %lf", &cap, &status, &min_step) != 3) return 2;
    if (cap < 0) return 2;
    int m = n < cap ? n : cap;
    m = m < 0 ? 0 : m;
    std::vector<double> s((size_t)m * 4), up((size_t)m * 4);
    for (std::vector<double>* v : {&s, &up})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    if (status <= 0) m = 0;
    std::printf("%d ", m);
    // forward: :1578-1603
    std::vector<int> source(m, -1);
    std::vector<double> heading(m, 0.0);
    for (int i = 0; i < m; ++i) {
      heading[i] = s[(size_t)i * 4 + 3];
      if (i + 1 >= m) break;
      const hq::Step st = hq::step_xy(&s[(size_t)i * 4], &s[(size_t)i * 4 + 4]);
      if (hq::is_source(i, st.dist, min_step)) {
        heading[i] = hq::heading_of(st.dx, st.dy);
        source[i] = i;
      } else {
        heading[i] = heading[i - 1];
        source[i] = source[i - 1];
      }
    }
    for (int i = 0; i < m; ++i) std::printf("%d %.17g ", source[i], heading[i]);
    // backward: a source's sum over its run in increasing row index, then the two rows of its step
    std::vector<double> G(m, 0.0), ra((size_t)m * 2, 0.0), rb((size_t)m * 2, 0.0);
    for (int i = 0; i + 1 < m; ++i) G[source[i]] = hq::accumulate(G[source[i]], up[(size_t)i * 4 + 3]);
    for (int i = 0; i + 1 < m; ++i) {
      if (source[i] != i) continue;
      const hq::Step st = hq::step_xy(&s[(size_t)i * 4], &s[(size_t)i * 4 + 4]);
      double a[2], b[2];
      hq::atan2_rows(st.dx, st.dy, G[i], a, b);
      for (int k = 0; k < 2; ++k) ra[(size_t)i * 2 + k] = a[k], rb[(size_t)i * 2 + k] = b[k];
    }
    for (int i = 0; i < m; ++i) {
      double g[4] = {up[(size_t)i * 4], up[(size_t)i * 4 + 1], up[(size_t)i * 4 + 2], i == m - 1 ? up[(size_t)i * 4 + 3] : 0.0};
      for (int k = 0; k < 2; ++k) {
        if (i + 1 < m && source[i] == i) g[k] = hq::accumulate(g[k], ra[(size_t)i * 2 + k]);
        if (i > 0 && source[i - 1] == i - 1) g[k] = hq::accumulate(g[k], rb[(size_t)(i - 1) * 2 + k]);
      }
      std::printf("%.17g %.17g %.17g %.17g ", g[0], g[1], g[2], g[3]);
    }
    std::printf("\n");
  }
}

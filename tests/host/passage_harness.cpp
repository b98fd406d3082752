// passage_harness.cpp -- where a sampled trajectory passes its waypoints and the backward pass of that
// (csrc/mrs_tg_passage.hpp: the distance, the foot point, the gradient rows and the reference loops waypoint_passage_kernel /
// waypoint_passage_vjp_kernel are checked against) compiled with plain g++ for the CPU: the scan written as the reference writes
// it -- one step after the other -- and the sums in the order the header states.  tests/test_passage_host.py checks it against
// the oracle bit for bit and against 60-digit fixtures; tests/test_gpu_passage.py checks the kernels against it bit for bit.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/passage_harness.cpp -o passage_harness && ./passage_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   W n_samples capacity status, waypoints [W][3], samples [m][3] with m = min(n_samples, capacity), grad_miss [W],
//   grad_fraction [W]
// Output per path, one line: count; index [W]; miss [W]; fraction [W]; dL/dsamples [m][3]; dL/dwaypoints [W][3].
// status <= 0: nothing is scanned.  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_passage.hpp"

namespace pq = mrs_tg::passq;

int main() {
  for (;;) {
    int W = 0, n = 0, cap = 0, status = 0;
    if (std::scanf("%d", &W) != 1) return 0;
    if (std::scanf("%d %d %d", &n, &cap, &status) != 3) return 2;
    if (W < 0 || cap < 0) return 2;
    int m = n < cap ? n : cap;
    m = m < 0 ? 0 : m;
    std::vector<double> w((size_t)W * 3), s((size_t)m * 3), gm(W), gt(W);
    for (std::vector<double>* v : {&w, &s, &gm, &gt})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<int32_t> index(W);
    std::vector<double> miss(W), fraction(W), gs((size_t)m * 3), gw((size_t)W * 3);
    const int scanned = status > 0 ? m : 0;
    const int count = pq::scan(w.data(), W, 3, s.data(), scanned, 3, index.data(), miss.data(), fraction.data());
    pq::scan_vjp(w.data(), W, 3, s.data(), m, 3, index.data(), count, gm.data(), gt.data(), gs.data(), gw.data());
    std::printf("%d ", count);
    for (int32_t x : index) std::printf("%d ", x);
    for (const std::vector<double>* v : {&miss, &fraction, &gs, &gw})
      for (double x : *v) std::printf("%.17g ", x);
    std::printf("\n");
  }
}

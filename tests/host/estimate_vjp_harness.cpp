// estimate_vjp_harness.cpp -- the backward pass of the Euclidean segment-time estimate (csrc/mrs_tg_estimate_vjp.hpp: the
// classification, the partials and the two sums estimate_times_vjp_kernel runs) compiled with plain g++ for the CPU, one vertex
// and one path after the other.  tests/test_estimate_host.py checks it against the 60-digit fixtures of
// tests/golden/gen_estimate_cases.py; tests/test_gpu_estimate.py checks the kernel against it bit for bit.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/estimate_vjp_harness.cpp -o estimate_vjp_harness && ./estimate_vjp_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   S, waypoints [S + 1][4], limits [9], upstream [S]
// Output per path, one line: per segment its term and the forward's value; dL/dwaypoints [S + 1][4]; dL/dlimits [9].  Doubles
// are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_estimate_vjp.hpp"

namespace ev = mrs_tg::estvjp;

int main() {
  for (;;) {
    int S = 0;
    if (std::scanf("%d", &S) != 1) return 0;
    if (S < 1) return 2;
    std::vector<double> w((size_t)(S + 1) * 4), lim(ev::kLimits), G(S);
    for (std::vector<double>* v : {&w, &lim, &G})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<int> term(S, -1);
    std::vector<double> gw((size_t)(S + 1) * 4);
    for (int j = 0; j <= S; ++j) {  // the kernel's vertex lanes
      const double* row = w.data() + (size_t)j * 4;
      double g[4];
      ev::vertex_gradient(j > 0 ? row - 4 : nullptr, j > 0 ? G[j - 1] : 0.0, j < S ? row : nullptr, j < S ? G[j] : 0.0, lim.data(),
                          g, j < S ? &term[j] : nullptr);
      for (int k = 0; k < 4; ++k) gw[(size_t)j * 4 + k] = g[k];
    }
    double gl[ev::kLimits];  // the kernel's path lane
    ev::limit_gradient(w.data(), G.data(), S, lim.data(), gl);
    for (int j = 0; j < S; ++j) std::printf("%d %.17g ", term[j], ev::classify(w.data() + (size_t)j * 4, lim.data()).value);
    for (double x : gw) std::printf("%.17g ", x);
    for (double x : gl) std::printf("%.17g ", x);
    std::printf("\n");
  }
}

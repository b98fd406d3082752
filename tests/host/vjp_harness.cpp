// vjp_harness.cpp -- the backward pass of the fixed-times solve (csrc/mrs_tg_vjp.hpp, the per-lane routine vjp_kernel runs)
// compiled with plain g++ for the CPU, so that the arithmetic can be checked against the 60-digit fixtures and a dense torch
// restatement without a GPU (tests/test_vjp_host.py).
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/vjp_harness.cpp -o vjp_harness && ./vjp_harness < cases.txt
//
// Input (whitespace separated), any number of cases until end of input: d S, seg_times[S], fixed_mask[(S + 1) * 5],
// fixed_values[(S + 1) * 5 * 4], coeffs [S][4][10], has_grad_coeffs (0: NULL), grad_coeffs [S][4][10] (read either way),
// grad_cost.  Output per case: dL/dfixed_values [(S + 1) * 5 * 4] on one line, dL/dseg_times [S] on the next; the time
// gradient of a segment is summed over the dimensions as the kernel's quad does, (dim 0 + dim 1) + (dim 2 + dim 3).
// The workspace and the outputs are filled with quiet NaNs before every lane, as a recycled device block may hold anything:
// every element the routine reads must be one it wrote, and every output element must be written.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_vjp.hpp"

namespace vj = mrs_tg::vjp;

int main() {
  int d = 0, S = 0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  while (std::scanf("%d %d", &d, &S) == 2) {
    if (S < 1 || d < 0 || d > 4) return 2;
    const size_t V = (size_t)S + 1;
    std::vector<double> times(S), vals(V * 5 * 4), coeffs((size_t)S * 4 * 10), gc((size_t)S * 4 * 10);
    std::vector<uint8_t> mask(V * 5);
    for (double& t : times)
      if (std::scanf("%lf", &t) != 1) return 2;
    for (uint8_t& m : mask) {
      int x = 0;
      if (std::scanf("%d", &x) != 1) return 2;
      m = (uint8_t)(x != 0);
    }
    for (double& v : vals)
      if (std::scanf("%lf", &v) != 1) return 2;
    for (double& c : coeffs)
      if (std::scanf("%lf", &c) != 1) return 2;
    int has_gc = 0;
    if (std::scanf("%d", &has_gc) != 1) return 2;
    for (double& c : gc)
      if (std::scanf("%lf", &c) != 1) return 2;
    double g = 0.0;
    if (std::scanf("%lf", &g) != 1) return 2;
    std::vector<double> ws(V * vj::kWsPerVertex), gv(V * 5 * 4, nan), tg((size_t)4 * S, nan);
    for (int dim = 0; dim < 4; ++dim) {
      for (double& x : ws) x = nan;
      double* tgd = tg.data() + (size_t)dim * S;
      vj::vjp_lane(mask.data(), vals.data(), 0, S, d, dim, times.data(), coeffs.data(), has_gc ? gc.data() : nullptr, g,
                   vj::LaneWs{ws.data(), 1}, gv.data(), [tgd](int i, double x) { tgd[i] = x; });
    }
    for (double x : gv) std::printf("%.17g ", x);
    std::printf("\n");
    for (int i = 0; i < S; ++i) std::printf("%.17g ", (tg[i] + tg[S + i]) + (tg[2 * S + i] + tg[3 * S + i]));
    std::printf("\n");
  }
  return 0;
}

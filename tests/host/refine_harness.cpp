// refine_harness.cpp -- the refinement pass of MRS_TG_FLAG_REFINE (csrc/mrs_tg_refine.hpp, the per-lane routine the refine
// kernel runs) compiled with plain g++ for the CPU, so that the arithmetic can be checked against the 60-digit fixtures
// without a GPU (tests/test_refine_tables.py).
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/refine_harness.cpp -o refine_harness && ./refine_harness < case.txt
//
// Input (whitespace separated): d S, then seg_times[S], fixed_mask[(S + 1) * 5], fixed_values[(S + 1) * 5 * 4] and the
// coefficients to refine [S][4][10].  Output: the refined coefficients (one line), the cost, the accepted steps per dimension,
// and per dimension 1 if the guard stopped it (a step that did not lower the residual), else 0.
// The workspace is filled with quiet NaNs before every lane, as a recycled device block may hold anything: every element the
// routine reads must be one it wrote.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_refine.hpp"

namespace rf = mrs_tg::refine;

int main() {
  int d = 0, S = 0;
  if (std::scanf("%d %d", &d, &S) != 2 || S < 1 || d < 0 || d > 4) return 2;
  std::vector<double> times(S), vals((size_t)(S + 1) * 5 * 4), coeffs((size_t)S * 4 * 10);
  std::vector<uint8_t> mask((size_t)(S + 1) * 5);
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
  std::vector<double> ws((size_t)(S + 1) * rf::kWsPerVertex);
  rf::dd cost{0.0, 0.0};
  rf::RefineOutcome out[4];
  for (int dim = 0; dim < 4; ++dim) {
    for (double& x : ws) x = std::numeric_limits<double>::quiet_NaN();
    rf::dd c{0.0, 0.0};
    out[dim] = rf::refine_lane(mask.data(), vals.data(), 0, S, d, dim, times.data(), coeffs.data(), rf::LaneWs{ws.data(), 1}, c);
    cost = rf::dd_add(cost, c);
  }
  for (double c : coeffs) std::printf("%.17g ", c);
  std::printf("\n%.17g\n%d %d %d %d\n%d %d %d %d\n", cost.hi + cost.lo, out[0].steps, out[1].steps, out[2].steps, out[3].steps,
              out[0].refused, out[1].refused, out[2].refused, out[3].refused);
  return 0;
}

// maxima_vjp_harness.cpp -- the backward pass of the segment maxima (csrc/mrs_tg_maxima_vjp.hpp, the per-entry routine and the
// segment sums segment_maxima_vjp_kernel runs) compiled with plain g++ for the CPU, so that the refinement and the envelope
// gradients can be checked against the 60-digit fixtures without a GPU (tests/test_maxima_vjp_host.py).  The forward's
// search is not part of it: every entry's seed abscissa and grid cell are inputs.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/maxima_vjp_harness.cpp -o maxima_vjp_harness && ./maxima_vjp_harness < in
//
// Input (whitespace separated), any number of segments until end of input: coeffs [4][10], T, then per entry
// w = 3 (k-1) + group, w = 0..8: tau_seed lo hi G (tau = t / T; [lo, hi] the seed's grid cell; G = dL/dM).  Output per
// segment, one line: dL/dcoeffs [40], dL/dT, t* [9] in seconds.  A segment the kernel would give zero rows (T <= 0, a
// non-finite T or coefficient) gives zeros here too.  The outputs are filled with quiet NaNs first: every element must be
// written.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_maxima_vjp.hpp"

namespace mv = mrs_tg::maxvjp;

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> c(mv::kD * mv::kN);
  for (;;) {
    for (double& x : c)
      if (std::scanf("%lf", &x) != 1) return 0;
    double T = 0.0, seed[mv::kEntries][4];
    if (std::scanf("%lf", &T) != 1) return 2;
    for (auto& s : seed)
      for (double& x : s)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<mv::EntryTerms> terms(mv::kEntries, mv::EntryTerms{nan, nan, nan, nan});
    std::vector<double> gc(mv::kD * mv::kN, nan), tstar(mv::kEntries, nan);
    double gT = nan;
    bool ok = true;
    for (int w = 0; w < mv::kEntries; ++w) ok = mv::entry_valid(c.data(), T, w) && ok;
    for (int w = 0; w < mv::kEntries; ++w)
      terms[w] = ok ? mv::entry_terms(c.data(), T, w, seed[w][0], seed[w][1], seed[w][2], seed[w][3])
                    : mv::EntryTerms{0.0, 0.0, 0.0, 0.0};
    for (int dim = 0; dim < mv::kD; ++dim)
      for (int j = 0; j < mv::kN; ++j) gc[dim * mv::kN + j] = ok ? mv::coeff_gradient(terms.data(), 1, dim, j) : 0.0;
    gT = ok ? mv::time_gradient(terms.data(), 1) : 0.0;
    for (int w = 0; w < mv::kEntries; ++w) tstar[w] = ok ? terms[w].t : 0.0;
    for (double x : gc) std::printf("%.17g ", x);
    std::printf("%.17g ", gT);
    for (double x : tstar) std::printf("%.17g ", x);
    std::printf("\n");
  }
}

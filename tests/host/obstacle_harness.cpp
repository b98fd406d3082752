// obstacle_harness.cpp -- the clearance from static obstacles and its backward pass (csrc/mrs_tg_obstacle.hpp: the clamped set
// bounds, the signed distance, the running minimum and the row gradient obstacle_clearance_kernel / obstacle_clearance_vjp_kernel
// run) compiled with plain g++ for the CPU, with the stage written as its contract states it -- per row the obstacles of the
// path's set one after the other in increasing index.  tests/test_obstacle_host.py checks it against the numpy and torch
// restatements of tests/obstacle_util.py; tests/test_gpu_obstacle.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/obstacle_harness.cpp -o obstacle_harness && ./obstacle_harness < in
//
// Input (whitespace separated), any number of batches until end of input:
//   n_paths capacity n_obstacles n_sets z_scale with_path_set with_nearest, set_offsets [n_sets + 1], with with_path_set != 0
//   path_set [n_paths] (else: the null pointer), n_samples [n_paths], status [n_paths], obstacles [n_obstacles][4], samples
//   [n_paths][capacity][4], upstream [n_paths][capacity], and with with_nearest != 0 the nearest array [n_paths][capacity] the
//   backward pass is driven by (else: the forward's).
// The offsets, the path_set and the nearest entries may be anything: negative, decreasing, beyond n_obstacles, out of the set.
// Output per path, one line: clearance [capacity], nearest [capacity], the path's minimum, its row and that row's obstacle,
// dL/dsamples [capacity][4], and the number of (row, obstacle) pairs of the path whose square root obsq::cannot_win would have
// spared.  Doubles are printed with 17 significant digits: the bits survive.
// Beside the plain loop the harness walks every row a second time with obsq::cannot_win against the running minimum, and
// against the minimum as it stood four obstacles earlier (the kernel's use of it), leaving out what the test lets it leave
// out: exit code 3 if that ever gives another minimum or another index than the plain loop.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_obstacle.hpp"

namespace oq = mrs_tg::obsq;

int main() {
  for (;;) {
    int P = 0, cap = 0, M = 0, S = 0, with_path_set = 0, with_nearest = 0;
    double z_scale = 1.0;
    if (std::scanf("%d", &P) != 1) return 0;
    if (std::scanf("%d %d %d %lf %d %d", &cap, &M, &S, &z_scale, &with_path_set, &with_nearest) != 6) return 2;
    if (P < 0 || cap < 0 || M < 0 || S < 0) return 2;
    std::vector<int32_t> off((size_t)S + 1), path_set(with_path_set ? P : 0), ns(P), status(P);
    for (std::vector<int32_t>* v : {&off, &path_set, &ns, &status})
      for (int32_t& x : *v)
        if (std::scanf("%d", &x) != 1) return 2;
    std::vector<double> ob((size_t)M * 4), s((size_t)P * cap * 4), up((size_t)P * cap);
    for (std::vector<double>* v : {&ob, &s, &up})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<int32_t> nearest((size_t)P * cap, -1), driven((size_t)P * cap, -1);
    if (with_nearest)
      for (int32_t& x : driven)
        if (std::scanf("%d", &x) != 1) return 2;
    const int32_t* ps = with_path_set ? path_set.data() : nullptr;
    std::vector<int> n(P);
    for (int p = 0; p < P; ++p) n[p] = oq::live_rows(status[p] > 0, ns[p], cap);
    auto row = [&](int p, int r) { return &s[((size_t)p * cap + r) * 4]; };
    // forward
    std::vector<double> clearance((size_t)P * cap, oq::no_clearance());
    std::vector<oq::Nearest> least(P, oq::nearest_none());
    std::vector<int> least_nearest(P, -1);
    std::vector<long long> spared(P, 0);
    for (int p = 0; p < P; ++p) {
      const oq::Bounds b = oq::path_obstacles(off.data(), S, ps, p, M);
      for (int r = 0; r < n[p]; ++r) {
        const oq::Nearest m = oq::nearest_obstacle(row(p, r), ob.data(), b, z_scale);
        oq::Nearest lean = oq::nearest_none(), stale = oq::nearest_none();
        double older = oq::no_clearance();  // the minimum of `stale` at the last multiple of four obstacles
        for (int k = b.begin; k < b.end; ++k) {
          const double* o = &ob[(size_t)k * 4];
          const double q = oq::distance_squared(row(p, r), o, z_scale);
          if (oq::cannot_win(q, lean.c, o[3])) ++spared[p];
          else oq::take(lean, oq::clearance_from(q, o[3]), k);
          if ((k - b.begin) % 4 == 0) older = stale.c;
          if (!oq::cannot_win(q, older, o[3])) oq::take(stale, oq::clearance_from(q, o[3]), k);
        }
        for (const oq::Nearest* other : {&lean, &stale})
          if (other->index != m.index || !(other->c == m.c || (other->c != other->c && m.c != m.c))) return 3;
        clearance[(size_t)p * cap + r] = m.c;
        nearest[(size_t)p * cap + r] = m.index;
        if (m.c < least[p].c) least[p].c = m.c, least[p].index = r, least_nearest[p] = m.index;
      }
    }
    if (!with_nearest) driven = nearest;
    // backward: one row, one term
    std::vector<double> grad((size_t)P * cap * 4, 0.0);
    for (int p = 0; p < P; ++p) {
      const oq::Bounds b = oq::path_obstacles(off.data(), S, ps, p, M);
      for (int r = 0; r < n[p]; ++r) {
        double gi[3];
        oq::row_gradient(row(p, r), ob.data(), b, driven[(size_t)p * cap + r], z_scale, up[(size_t)p * cap + r], gi);
        for (int k = 0; k < 3; ++k) grad[((size_t)p * cap + r) * 4 + k] = gi[k];
      }
    }
    for (int p = 0; p < P; ++p) {
      for (int r = 0; r < cap; ++r) std::printf("%.17g ", clearance[(size_t)p * cap + r]);
      for (int r = 0; r < cap; ++r) std::printf("%d ", nearest[(size_t)p * cap + r]);
      std::printf("%.17g %d %d ", least[p].c, least[p].index, least_nearest[p]);
      for (size_t e = 0; e < (size_t)cap * 4; ++e) std::printf("%.17g ", grad[(size_t)p * cap * 4 + e]);
      std::printf("%lld ", spared[p]);
      std::printf("\n");
    }
  }
}

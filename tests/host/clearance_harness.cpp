// clearance_harness.cpp -- the mutual clearance within groups of paths and its backward pass (csrc/mrs_tg_clearance.hpp: the
// group bounds, the live-row-at-step test, the distance, the running minimum and the two gradient rows mutual_clearance_kernel /
// mutual_clearance_vjp_kernel run) compiled with plain g++ for the CPU, with the stage written as its contract states it -- per
// row the group's other paths one after the other in increasing index, the backward pass a gather in the order the header
// states.  tests/test_clearance_host.py checks it against the numpy and torch restatements of tests/clearance_util.py;
// tests/test_gpu_clearance.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/clearance_harness.cpp -o clearance_harness && ./clearance_harness < in
//
// Input (whitespace separated), any number of batches until end of input:
//   n_paths capacity n_groups z_scale with_partner, group_offsets [n_groups + 1], n_samples [n_paths], status [n_paths],
//   first_step [n_paths], samples [n_paths][capacity][4], upstream [n_paths][capacity], and with with_partner != 0 the partner
//   array [n_paths][capacity] the backward pass is driven by (else: the forward's).
// The offsets and the partner entries may be anything: negative, decreasing, beyond n_paths, out of group.
// Output per path, one line: clearance [capacity], partner [capacity], the path's minimum, its row and that row's partner,
// dL/dsamples [capacity][4].  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_clearance.hpp"

namespace cq = mrs_tg::clrq;

int main() {
  for (;;) {
    int P = 0, cap = 0, G = 0, with_partner = 0;
    double z_scale = 1.0;
    if (std::scanf("%d", &P) != 1) return 0;
    if (std::scanf("%d %d %lf %d", &cap, &G, &z_scale, &with_partner) != 4) return 2;
    if (P < 0 || cap < 0 || G < 0) return 2;
    std::vector<int32_t> off((size_t)G + 1), ns(P), status(P), first(P);
    for (std::vector<int32_t>* v : {&off, &ns, &status, &first})
      for (int32_t& x : *v)
        if (std::scanf("%d", &x) != 1) return 2;
    std::vector<double> s((size_t)P * cap * 4), up((size_t)P * cap);
    for (std::vector<double>* v : {&s, &up})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<int32_t> partner((size_t)P * cap, -1), driven((size_t)P * cap, -1);
    if (with_partner)
      for (int32_t& x : driven)
        if (std::scanf("%d", &x) != 1) return 2;
    std::vector<int> n(P);
    for (int p = 0; p < P; ++p) n[p] = cq::live_rows(status[p] > 0, ns[p], cap);
    auto row = [&](int p, int r) { return &s[((size_t)p * cap + r) * 4]; };
    // forward
    std::vector<double> clearance((size_t)P * cap, cq::no_clearance());
    std::vector<cq::Nearest> least(P, cq::nearest_none());
    std::vector<int> least_partner(P, -1);
    for (int p = 0; p < P; ++p) {
      const cq::Bounds gb = cq::group_of(off.data(), G, p, P);
      for (int r = 0; r < n[p]; ++r) {
        const long long step = cq::step_of(first[p], r);
        cq::Nearest m = cq::nearest_none();
        for (int j = gb.begin; j < gb.end; ++j) {
          if (j == p) continue;
          const int rj = cq::row_at_step(step, first[j], n[j]);
          if (rj >= 0) cq::take(m, cq::distance(row(p, r), row(j, rj), z_scale), j);
        }
        clearance[(size_t)p * cap + r] = m.c;
        partner[(size_t)p * cap + r] = m.index;
        if (m.c < least[p].c) least[p].c = m.c, least[p].index = r, least_partner[p] = m.index;
      }
    }
    if (!with_partner) driven = partner;
    // backward: a gather -- the row's own term, then the rows that name it, in increasing path index
    std::vector<double> grad((size_t)P * cap * 4, 0.0);
    for (int j = 0; j < P; ++j) {
      const cq::Bounds gb = cq::group_of(off.data(), G, j, P);
      for (int r = 0; r < n[j]; ++r) {
        const long long step = cq::step_of(first[j], r);
        double acc[3] = {0.0, 0.0, 0.0}, gi[3], gj[3];
        const int q = driven[(size_t)j * cap + r];
        if (cq::partner_in_group(q, j, gb)) {
          const int rq = cq::row_at_step(step, first[q], n[q]);
          if (rq >= 0) {
            cq::row_vjp(row(j, r), row(q, rq), z_scale, up[(size_t)j * cap + r], gi);
            for (int k = 0; k < 3; ++k) acc[k] = cq::accumulate(acc[k], gi[k]);
          }
        }
        for (int i = gb.begin; i < gb.end; ++i) {
          if (i == j) continue;
          const int ri = cq::row_at_step(step, first[i], n[i]);
          if (ri < 0 || driven[(size_t)i * cap + ri] != j) continue;
          cq::row_vjp(row(i, ri), row(j, r), z_scale, up[(size_t)i * cap + ri], gi);
          cq::partner_row(gi, gj);
          for (int k = 0; k < 3; ++k) acc[k] = cq::accumulate(acc[k], gj[k]);
        }
        for (int k = 0; k < 3; ++k) grad[((size_t)j * cap + r) * 4 + k] = acc[k];
      }
    }
    for (int p = 0; p < P; ++p) {
      for (int r = 0; r < cap; ++r) std::printf("%.17g ", clearance[(size_t)p * cap + r]);
      for (int r = 0; r < cap; ++r) std::printf("%d ", partner[(size_t)p * cap + r]);
      std::printf("%.17g %d %d ", least[p].c, least[p].index, least_partner[p]);
      for (size_t e = 0; e < (size_t)cap * 4; ++e) std::printf("%.17g ", grad[(size_t)p * cap * 4 + e]);
      std::printf("\n");
    }
  }
}

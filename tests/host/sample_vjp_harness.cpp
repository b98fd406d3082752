// sample_vjp_harness.cpp -- the backward pass of the sampler (csrc/mrs_tg_sample_vjp.hpp, the per-term routines and the sums
// sample_vjp_kernel runs, in its order) compiled with plain g++ for the CPU, so that the gradients can be checked against the
// 60-digit fixtures without a GPU (tests/test_sample_vjp_host.py).  The walk is a serial restatement of the reference's
// accumulate-and-carry loop written here (the kernel runs the forward's wavefront-wide chunked walk, which produces the same
// additions in the same order).
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/sample_vjp_harness.cpp -o sample_vjp_harness && ./sample_vjp_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   S n_orders capacity status dt, T [S], coeffs [S][4][10], R, upstream rows [R][n_orders][4]   (R >= min(n, capacity))
// Output per path, one line: n (capacity + 1 = more than fit), then per sample k < min(n, capacity) its segment and time in
// segment, then dL/dcoeffs [S][40] and dL/dseg_times [S].  status <= 0: zero rows.  Outputs and scratch are filled with quiet
// NaNs before every path: every element must be written, and nothing may be read that was not.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_sample_vjp.hpp"

namespace sv = mrs_tg::sampvjp;

template <int NO>
static void backward(int S, const std::vector<double>& c, const std::vector<double>& G, const std::vector<int>& seg,
                     const std::vector<double>& tin, bool live, std::vector<double>& gc, std::vector<double>& gT) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int kTime = NO * sv::kD;
  std::vector<double> s_sum(S, nan);
  double acc[sv::kCoeffElems + kTime];
  double wc[sv::kN][sv::kN], wt[NO][sv::kN];
  for (int j = 0; j < sv::kN; ++j) sv::coeff_weights(j, wc[j]);
  for (int o = 0; o < NO; ++o) sv::time_weights(o, wt[o]);
  int cur = -1;
  auto close_segments = [&](int next) {
    if (cur >= 0) {
      for (int e = 0; e < sv::kCoeffElems; ++e) gc[(size_t)cur * sv::kCoeffElems + e] = acc[e];
      double s = acc[sv::kCoeffElems];
      for (int r = 1; r < kTime; ++r) s = sv::accumulate(s, acc[sv::kCoeffElems + r]);
      s_sum[cur] = s;
    }
    for (int i = cur + 1; i < next; ++i) {
      for (int e = 0; e < sv::kCoeffElems; ++e) gc[(size_t)i * sv::kCoeffElems + e] = 0.0;
      s_sum[i] = 0.0;
    }
  };
  if (live) {
    for (size_t k = 0; k < seg.size(); ++k) {
      if (seg[k] != cur) {
        close_segments(seg[k]);
        cur = seg[k];
        for (double& a : acc) a = 0.0;
      }
      const double* row = G.data() + k * kTime;
      const double t = tin[k];
      for (int e = 0; e < sv::kCoeffElems; ++e) {
        const int dim = e / sv::kN, j = e % sv::kN;
        double g[NO];
        for (int o = 0; o < NO; ++o) g[o] = row[o * sv::kD + dim];
        acc[e] = sv::accumulate(acc[e], sv::coeff_term<NO>(j, wc[j], g, t));
      }
      for (int r = 0; r < kTime; ++r) {
        const int o = r / sv::kD, dim = r % sv::kD;
        const double* cd = c.data() + (size_t)cur * sv::kCoeffElems + dim * sv::kN;
        acc[sv::kCoeffElems + r] = sv::accumulate(acc[sv::kCoeffElems + r], sv::time_term(o, wt[o], cd, row[r], t));
      }
    }
  }
  close_segments(S);
  sv::time_gradients(s_sum.data(), S, gT.data());
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (;;) {
    int S = 0, n_orders = 0, capacity = 0, status = 0, R = 0;
    double dt = 0.0;
    if (std::scanf("%d", &S) != 1) return 0;
    if (std::scanf("%d %d %d %lf", &n_orders, &capacity, &status, &dt) != 4) return 2;
    if (S < 1 || (n_orders != 1 && n_orders != sv::kMaxOrders) || capacity < 0) return 2;
    std::vector<double> T(S), c((size_t)S * sv::kCoeffElems);
    for (double& x : T)
      if (std::scanf("%lf", &x) != 1) return 2;
    for (double& x : c)
      if (std::scanf("%lf", &x) != 1) return 2;
    if (std::scanf("%d", &R) != 1 || R < 0) return 2;
    std::vector<double> G((size_t)R * n_orders * sv::kD);
    for (double& x : G)
      if (std::scanf("%lf", &x) != 1) return 2;
    // the walk: sample k is taken while the accumulated time (k additions of dt) is below the trajectory's end; the time in
    // the segment grows by dt and its excess over the segment's length is carried into the next segment(s)
    std::vector<int> seg;
    std::vector<double> tin_of;
    int n = 0;
    {
      double t_end = 0.0;
      for (int i = 0; i < S; ++i) t_end += T[i];
      int i = 0;
      double acc0 = 0.0;
      for (i = 0; i < S; ++i) {
        acc0 += T[i];
        if (acc0 > 0.0) break;
      }
      double tin = 0.0, accumulated = 0.0;
      while (i < S && accumulated < t_end) {
        while (i < S && tin > T[i]) {
          tin = tin - T[i];
          ++i;
        }
        if (i >= S) break;
        if (n < capacity) {
          seg.push_back(i);
          tin_of.push_back(tin);
        }
        ++n;
        if (n > capacity) break;
        tin += dt;
        accumulated += dt;
      }
    }
    if ((int)seg.size() > R) return 3;
    G.resize(seg.size() * (size_t)n_orders * sv::kD);  // (rows at or beyond the sample count are dropped unread)
    std::vector<double> gc((size_t)S * sv::kCoeffElems, nan), gT(S, nan);
    if (n_orders == 1)
      backward<1>(S, c, G, seg, tin_of, status > 0, gc, gT);
    else
      backward<sv::kMaxOrders>(S, c, G, seg, tin_of, status > 0, gc, gT);
    std::printf("%d ", n);
    for (size_t k = 0; k < seg.size(); ++k) std::printf("%d %.17g ", seg[k], tin_of[k]);
    for (double x : gc) std::printf("%.17g ", x);
    for (double x : gT) std::printf("%.17g ", x);
    std::printf("\n");
  }
}

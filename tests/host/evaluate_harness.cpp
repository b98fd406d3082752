// evaluate_harness.cpp -- the evaluation at caller-given times and its backward pass (csrc/mrs_tg_evaluate.hpp: the locate
// rule, the Horner rows and the per-query terms evaluate_kernel / evaluate_vjp_kernel run, summed in the kernel's order)
// compiled with plain g++ for the CPU, so that states and gradients can be checked against the 60-digit fixtures without a
// GPU (tests/test_evaluate_host.py).
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/evaluate_harness.cpp -o evaluate_harness && ./evaluate_harness < in
//
// Input (whitespace separated), any number of paths until end of input:
//   S n_orders n_queries status, T [S], coeffs [S][4][10], query times [n_queries], upstream rows [n_queries][n_orders][4]
// Output per path, one line: per query its segment (-1 = out of range), its local time and its state row [n_orders][4];
// then dL/dcoeffs [S][40], dL/dseg_times [S] and dL/dquery_times [n_queries].  status <= 0: zero gradient rows.  Outputs are
// filled with quiet NaNs before every path: every element must be written.  Exit code 4: the bisection over the running sums
// and the loop as the reference writes it disagreed on a query.
#include <cstdio>
#include <limits>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_evaluate.hpp"

namespace ev = mrs_tg::evalq;
namespace sv = mrs_tg::sampvjp;

template <int NO>
static int run(int S, int nq, bool live, const std::vector<double>& T, const std::vector<double>& c,
               const std::vector<double>& tq, const std::vector<double>& G) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int kRow = NO * ev::kD, kStride = ev::kCoeffElems + 1;
  std::vector<double> A(S, nan), acc((size_t)S * kStride, 0.0), gq(nq, nan), gc((size_t)S * ev::kCoeffElems, nan), gT(S, nan);
  const bool sorted = ev::running_sums(T.data(), S, A.data());
  for (int q = 0; q < nq; ++q) {
    const ev::Located at = ev::locate(T.data(), A.data(), S, sorted, tq[q]);
    const ev::Located loop = ev::locate(T.data(), A.data(), S, false, tq[q]);
    if (at.seg != loop.seg || !(at.tau == loop.tau)) return 4;
    double row[NO][ev::kD];
    if (at.seg >= 0) {
      ev::state_row<NO>(c.data() + (size_t)at.seg * ev::kCoeffElems, at.tau, row);
    } else {
      for (int o = 0; o < NO; ++o)
        for (int dd = 0; dd < ev::kD; ++dd) row[o][dd] = 0.0;
    }
    std::printf("%d %.17g ", at.seg, at.tau);
    for (int o = 0; o < NO; ++o)
      for (int dd = 0; dd < ev::kD; ++dd) std::printf("%.17g ", row[o][dd]);
    if (!live || at.seg < 0) {
      gq[q] = 0.0;
      continue;
    }
    const double* up = G.data() + (size_t)q * kRow;  // (never touched for an out-of-range query)
    double terms[ev::kCoeffElems];
    ev::coeff_terms<NO>(up, at.tau, terms);
    const double g = ev::time_gradient<NO>(c.data() + (size_t)at.seg * ev::kCoeffElems, up, at.tau);
    gq[q] = g;
    double* a = acc.data() + (size_t)at.seg * kStride;
    for (int e = 0; e < ev::kCoeffElems; ++e) a[e] = sv::accumulate(a[e], terms[e]);
    a[ev::kCoeffElems] = sv::accumulate(a[ev::kCoeffElems], g);
  }
  std::vector<double> s(S);
  for (int i = 0; i < S; ++i) {
    for (int e = 0; e < ev::kCoeffElems; ++e) gc[(size_t)i * ev::kCoeffElems + e] = acc[(size_t)i * kStride + e];
    s[i] = acc[(size_t)i * kStride + ev::kCoeffElems];
  }
  sv::time_gradients(s.data(), S, gT.data());
  for (double x : gc) std::printf("%.17g ", x);
  for (double x : gT) std::printf("%.17g ", x);
  for (double x : gq) std::printf("%.17g ", x);
  std::printf("\n");
  return 0;
}

int main() {
  for (;;) {
    int S = 0, n_orders = 0, nq = 0, status = 0;
    if (std::scanf("%d", &S) != 1) return 0;
    if (std::scanf("%d %d %d", &n_orders, &nq, &status) != 3) return 2;
    if (S < 1 || (n_orders != 1 && n_orders != ev::kMaxOrders) || nq < 0) return 2;
    std::vector<double> T(S), c((size_t)S * ev::kCoeffElems), tq(nq), G((size_t)nq * n_orders * ev::kD);
    for (std::vector<double>* v : {&T, &c, &tq, &G})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    const int rc = n_orders == 1 ? run<1>(S, nq, status > 0, T, c, tq, G) : run<ev::kMaxOrders>(S, nq, status > 0, T, c, tq, G);
    if (rc != 0) return rc;
  }
}

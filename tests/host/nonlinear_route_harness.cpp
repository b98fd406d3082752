// nonlinear_route_harness.cpp -- the route of the Mellinger outer loop (csrc/mrs_tg_nonlinear_route.hpp: the LDS footprints, the
// lane-group bins of a plan by nonlinear_host_plan, the predicates, route_nonlinear) compiled with plain g++ for the CPU.  The knobs
// are read from the process's environment, most of them once: one process per setting.  tests/test_nonlinear_route_host.py drives
// it and restates, from the fields printed here, the kernel names launch_nonlinear notes (tests/nonlinear_route_util.py).
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/nonlinear_route_harness.cpp -o nonlinear_route_harness && ./nonlinear_route_harness < in
//
// Input: per request fifteen integers
//   derivative (the objective order)   constrained_slots moving_starts shared_device (the hints)   compute_units resident_blocks
//   estimate general careful samples_wanted   fused factor_store waypoints solve_compute_units (the closing request)   n_runs
// then the batch in the caller's path order as n_runs pairs (count, segments).  The plan's order is built here: longest first,
// stable.  A negative n_runs: -n_runs pairs, longest first, each of which is made a bin of the plan as it stands (a group of 64
// lanes, in bins, wide_bins and ends_bins alike) -- the only way to a plan of more bins than a launch's table holds.
// Output: three lines per request, fields by name.  The first: of the plan plan_dim_split regroup_possible wide_blocks and the
// bin lists bins bins1 wide_bins ends_bins (group:q_begin:q_count:max_S:min_S, comma-separated, - when empty); of the route
// dim_split estimate_in_kernel lean lean_kernel queued wave sweep_fits sweep_kernel careful general certified_maxima closing
// tail_samples and per launch (lean_, sweep_) bins (group:q_begin:q_count:max_S:block_begin), blocks, threads, lds; then
// gradient_lds (the largest launch of launch_cost_gradient), listed_lds (optimize_careful_kernel, optimize_general_kernel),
// lds_limit and lds_default.  The second and third: the closing solves' routes (solve_route_print.hpp).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_nonlinear_route.hpp"
#include "solve_route_print.hpp"

using namespace mrs_tg;

static std::string text(const std::vector<NonlinearBin>& bins) {
  std::string s;
  for (const NonlinearBin& b : bins) {
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s%d:%d:%d:%d:%d", s.empty() ? "" : ",", b.group, b.q_begin, b.q_count, b.max_S, b.min_S);
    s += buf;
  }
  return s.empty() ? "-" : s;
}

static std::string text(const BinTable& t) {
  std::string s;
  for (int i = 0; i < t.n; ++i) {
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s%d:%d:%d:%d:%d", i ? "," : "", t.group[i], t.q_begin[i], t.q_count[i], t.max_S[i], t.block_begin[i]);
    s += buf;
  }
  return s.empty() ? "-" : s;
}

int main() {
  int v[15];
  for (;;) {
    for (int i = 0; i < 15; ++i)
      if (std::scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 1;
    std::vector<int32_t> so(1, 0);
    std::vector<NonlinearBin> given;  // n_runs < 0: the plan's bins as written, every run a bin of its own
    for (int r = 0; r < std::abs(v[14]); ++r) {
      int count, S;
      if (std::scanf("%d %d", &count, &S) != 2 || count < 0 || S < 1) return 1;
      if (v[14] < 0) given.push_back(NonlinearBin{64, (int)so.size() - 1, count, S, S});
      for (int k = 0; k < count; ++k) so.push_back(so.back() + S);
    }
    const int P = (int)so.size() - 1;
    auto len = [&](int p) { return so[p + 1] - so[p]; };
    std::vector<int32_t> order(P);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return len(a) > len(c); });
    BatchView b{};
    b.n_paths = P;
    b.n_segments = so.back();
    b.max_segments = P > 0 ? len(order[0]) : 0;
    b.uniform_S = (P > 0 && len(order[P - 1]) == b.max_segments) ? b.max_segments : 0;
    RouteHints hints;
    hints.constrained_slots = v[1] != 0;
    hints.moving_starts = v[2] != 0;
    hints.shared_device = v[3] != 0;
    SolveRequest closing;
    closing.derivative = v[0];
    closing.hints = hints;
    closing.fused = v[10] != 0;
    closing.factor_store = v[11] != 0;
    closing.waypoints = v[12] != 0;
    closing.compute_units = v[13];

    NonlinearHostPlan nl = nonlinear_host_plan(so, order);
    if (!given.empty()) {  // (a table of more than five bins: no batch gives nonlinear_host_plan one, there are five group widths)
      nl.bins = nl.wide_bins = nl.ends_bins = given;
      nl.wide_blocks = (int)so.size() - 1;
    }
    const NonlinearRoute r = route_nonlinear(nl, b, hints, v[4], v[5], closing, v[6] != 0, v[7] != 0, v[8] != 0, v[9] != 0);

    static const char* const lean_names[] = {"lean", "lean_masked", "lean_shared", "lean_shared_ends", "lean_shared_ends_long"};
    static const char* const sweep_names[] = {"wave", "split", "compact", "compact_masked"};
    static const char* const closing_names[] = {"rows_pipeline", "quad_tail", "rows_tail", "separate"};
    const bool split = nl.dim_split == 4;
    size_t gradient_lds = 0;
    for (const NonlinearBin& bin : nl.bins) gradient_lds = std::max(gradient_lds, gradient_lds_bytes(bin, split));
    std::printf("plan_dim_split=%d regroup_possible=%d wide_blocks=%d bins=%s bins1=%s wide_bins=%s ends_bins=%s ", nl.dim_split,
                (int)nl.regroup_possible, nl.wide_blocks, text(nl.bins).c_str(), text(nl.bins1).c_str(), text(nl.wide_bins).c_str(),
                text(nl.ends_bins).c_str());
    std::printf("dim_split=%d estimate_in_kernel=%d lean=%d lean_kernel=%s queued=%d wave=%d sweep_fits=%d sweep_kernel=%s careful=%d "
                "general=%d certified_maxima=%d closing=%s tail_samples=%d ",
                r.dim_split, (int)r.estimate_in_kernel, (int)r.lean, lean_names[(int)r.lean_kernel], (int)r.queued, (int)r.wave(),
                (int)r.sweep_fits, sweep_names[(int)r.sweep_kernel], (int)r.careful, (int)r.general, (int)r.certified_maxima,
                closing_names[(int)r.closing()], (int)r.tail_samples());
    std::printf("lean_bins=%s lean_blocks=%d lean_threads=%u lean_lds=%zu sweep_bins=%s sweep_blocks=%d sweep_threads=%u sweep_lds=%zu ",
                text(r.lean_launch.bins).c_str(), r.lean_launch.blocks, r.lean_launch.threads, r.lean_launch.lds_bytes,
                text(r.sweep_launch.bins).c_str(), r.sweep_launch.blocks, r.sweep_launch.threads, r.sweep_launch.lds_bytes);
    std::printf("gradient_lds=%zu listed_lds=%zu lds_limit=%zu lds_default=%zu\n", gradient_lds, listed_lds_bytes(b.max_segments),
                kLdsPerWorkgroup, kLdsDefaultLimit);
    print_solve_route(r.first_solve);
    print_solve_route(r.final_solve);
  }
}

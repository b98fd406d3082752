// solve_route_harness.cpp -- the route of the fixed-times solve (csrc/mrs_tg_solve_route.hpp: the LDS footprints and budgets, the
// predicates, SolveRequest -> SolveRoute by route_solve) compiled with plain g++ for the CPU.  The knobs are read from the
// process's environment, most of them once: one process per setting.  tests/test_solve_route_host.py drives it and restates,
// from the fields printed here, the kernel names the library notes.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/solve_route_harness.cpp -o solve_route_harness && ./solve_route_harness < in
//
// Input: one request per line, sixteen integers
//   n_paths max_segments uniform_S   derivative fused factor_store group waypoints   shared_device constrained_slots
//   compute_units   stage (0 fixed times, 1 closing)   scale_from_maxima maxima_in_launch sampling   force (0 none, 1 rows, 2 tile)
// Output: one line per request, the route's fields by name (solve_route_print.hpp)
#include <cstdio>

#include "solve_route_print.hpp"

using namespace mrs_tg;

int main() {
  int v[16];
  for (;;) {
    for (int i = 0; i < 16; ++i)
      if (std::scanf("%d", &v[i]) != 1) return i == 0 ? 0 : 1;
    BatchView b{};
    b.n_paths = v[0];
    b.max_segments = v[1];
    b.uniform_S = v[2];
    SolveRequest q;
    q.derivative = v[3];
    q.fused = v[4] != 0;
    q.factor_store = v[5] != 0;
    q.group = v[6];
    q.waypoints = v[7] != 0;
    q.hints.shared_device = v[8] != 0;
    q.hints.constrained_slots = v[9] != 0;
    q.compute_units = v[10];
    q.stage = v[11] ? SolveStage::kClosing : SolveStage::kFixedTimes;
    q.scale_from_maxima = v[12] != 0;
    q.maxima_in_launch = v[13] != 0;
    q.sampling = v[14] != 0;
    q.force = v[15] == 1 ? SolveFamily::kRows : v[15] == 2 ? SolveFamily::kTile : SolveFamily::kNone;
    const SolveRoute r = route_solve(b, q);
    print_solve_route(r);
  }
}

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
// Output: one line per request, the route's fields by name
//   family=none|duo|quad|rows|rows_pipeline|tile|lane group wp ends lean with_tail fused lanes_per_path per_workgroup grid_x grid_y
//   threads blocks_per_batch lds_bytes raise_lds_to loop_bits scales maxima_in_launch sampling, then budget= the LDS budget of the
//   route's family (0: the family has no dynamic LDS) and lds_limit= what a workgroup can have
#include <cstdio>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_solve_route.hpp"

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
    const char* family = "none";
    size_t budget = 0;
    switch (r.family) {
      case SolveFamily::kNone: break;
      case SolveFamily::kDuo: family = "duo"; budget = kQuadLdsBudget; break;
      case SolveFamily::kQuad: family = "quad"; budget = kQuadLdsBudget; break;
      case SolveFamily::kRows: family = "rows"; budget = kRowsLdsBudget; break;
      case SolveFamily::kRowsPipeline: family = "rows_pipeline"; budget = kRowsLdsBudget; break;
      case SolveFamily::kTile: family = "tile"; budget = kTileLdsBudget; break;
      case SolveFamily::kLane: family = "lane"; break;
    }
    std::printf("family=%s group=%d wp=%d ends=%d lean=%d with_tail=%d fused=%d lanes_per_path=%d per_workgroup=%d grid_x=%u grid_y=%u "
                "threads=%u blocks_per_batch=%d lds_bytes=%zu raise_lds_to=%zu loop_bits=%d scales=%d maxima_in_launch=%d sampling=%d "
                "budget=%zu lds_limit=%zu\n",
                family, r.group, (int)r.wp, (int)r.ends, (int)r.lean, (int)r.with_tail, (int)r.fused, r.lanes_per_path, r.per_workgroup,
                r.grid_x, r.grid_y, r.threads, r.blocks_per_batch, r.lds_bytes, r.raise_lds_to, r.loop_bits, (int)r.scales,
                (int)r.maxima_in_launch, (int)r.sampling, budget, kLdsPerWorkgroup);
  }
}

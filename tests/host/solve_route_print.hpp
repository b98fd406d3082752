// solve_route_print.hpp -- a SolveRoute as one line of fields by name, shared by solve_route_harness.cpp and
// nonlinear_route_harness.cpp (tests/solve_route_util.py parses it):
//   family=none|duo|quad|rows|rows_pipeline|tile|lane group wp ends lean with_tail fused lanes_per_path per_workgroup grid_x grid_y
//   threads blocks_per_batch lds_bytes raise_lds_to loop_bits scales maxima_in_launch sampling, then budget= the LDS budget of the
//   route's family (0: the family has no dynamic LDS) and lds_limit= what a workgroup can have
#pragma once
#include <cstdio>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_solve_route.hpp"

inline void print_solve_route(const mrs_tg::SolveRoute& r) {
  using namespace mrs_tg;
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

// batch_harness.cpp -- the batch addressing of csrc/mrs_tg_batch.hpp (which path a segment, a vertex or a launch position
// belongs to, where a path starts) compiled with plain g++ for the CPU: every index of a BatchView filled on the host goes
// through the functions the kernels call.  tests/test_batch_host.py compares the output with a linear scan of seg_offsets.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/batch_harness.cpp -o batch_harness && ./batch_harness < in
//
// Input (whitespace separated), any number of batches until end of input:
//   n_paths uniform_S, seg_offsets [n_paths + 1], order [n_paths]
// Output per batch, one line: path_of_segment [sum S]; path_of_vertex [sum S + n_paths]; per path first_segment, segments_of,
// first_vertex; per position p, s0, S, v0 of path_at.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_batch.hpp"

int main() {
  for (;;) {
    mrs_tg::BatchView b{};
    if (std::scanf("%d", &b.n_paths) != 1) return 0;
    if (std::scanf("%d", &b.uniform_S) != 1 || b.n_paths < 1) return 2;
    std::vector<int32_t> offsets((size_t)b.n_paths + 1), order((size_t)b.n_paths);
    for (std::vector<int32_t>* v : {&offsets, &order})
      for (int32_t& x : *v)
        if (std::scanf("%d", &x) != 1) return 2;
    b.n_segments = offsets.back();
    for (int p = 0; p < b.n_paths; ++p) b.max_segments = b.max_segments > offsets[p + 1] - offsets[p] ? b.max_segments : offsets[p + 1] - offsets[p];
    b.seg_offsets = offsets.data();
    b.order = order.data();
    for (int s = 0; s < b.n_segments; ++s) std::printf("%d ", mrs_tg::path_of_segment(b, s));
    for (int v = 0; v < b.n_segments + b.n_paths; ++v) std::printf("%d ", mrs_tg::path_of_vertex(b, v));
    for (int p = 0; p < b.n_paths; ++p) {
      const int seg0 = mrs_tg::first_segment(b, p);
      std::printf("%d %d %d ", seg0, mrs_tg::segments_of(b, p, seg0), mrs_tg::first_vertex(b, p));
    }
    for (int q = 0; q < b.n_paths; ++q) {
      const mrs_tg::PathRef r = mrs_tg::path_at(b, q);
      std::printf("%d %d %d %d ", r.p, r.s0, r.S, r.v0);
    }
    std::printf("\n");
  }
}

// field_harness.cpp -- the clearance from a voxel distance field and its backward pass (csrc/mrs_tg_field.hpp: the inside test and
// cell choice, the trilinear interpolant, the field's gradient, the cell's encoding and validation, the row gradient
// field_clearance_kernel / field_clearance_vjp_kernel run) compiled with plain g++ for the CPU, with the stage written as its
// contract states it -- row by row.  tests/test_field_host.py checks it against the numpy and torch restatements of
// tests/field_util.py; tests/test_gpu_field.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/field_harness.cpp -o field_harness && ./field_harness < in
//
// Input (whitespace separated), any number of batches until end of input:
//   n_paths capacity n_fields nx ny nz, ox oy oz, hx hy hz, outside_value, with_path_field with_cell; with with_path_field != 0
//   path_field [n_paths] (else: the null pointer), n_samples [n_paths], status [n_paths], fields [n_fields][nz][ny][nx], samples
//   [n_paths][capacity][4], upstream [n_paths][capacity], and with with_cell != 0 the cell array [n_paths][capacity] the backward
//   pass is driven by (else: the forward's).
// path_field and the cell entries may be anything: negative, beyond the array, in another path's grid, on an axis' last node.
// The fields vector has exactly n_fields nz ny nx elements, so a sanitizer build sees every read beyond it.
// Output per path, one line: clearance [capacity], cell [capacity], gradient [capacity][4], the path's minimum, its row and
// that row's cell, dL/dsamples [capacity][4].  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_field.hpp"

namespace fq = mrs_tg::fldq;

int main() {
  for (;;) {
    int P = 0, cap = 0, with_path_field = 0, with_cell = 0;
    fq::Geometry G;
    double outside = 0.0;
    if (std::scanf("%d", &P) != 1) return 0;
    if (std::scanf("%d %d %d %d %d", &cap, &G.n_fields, &G.n[0], &G.n[1], &G.n[2]) != 5) return 2;
    if (std::scanf("%lf %lf %lf %lf %lf %lf %lf", &G.o[0], &G.o[1], &G.o[2], &G.h[0], &G.h[1], &G.h[2], &outside) != 7) return 2;
    if (std::scanf("%d %d", &with_path_field, &with_cell) != 2) return 2;
    if (P < 0 || cap < 0 || G.n_fields < 0 || G.n[0] < 2 || G.n[1] < 2 || G.n[2] < 2) return 2;
    const size_t voxels = (size_t)G.n_fields * G.n[2] * G.n[1] * G.n[0];
    if (voxels > 2147483647u) return 2;
    std::vector<int32_t> path_field(with_path_field ? P : 0), ns(P), status(P);
    for (std::vector<int32_t>* v : {&path_field, &ns, &status})
      for (int32_t& x : *v)
        if (std::scanf("%d", &x) != 1) return 2;
    std::vector<double> fields(voxels), s((size_t)P * cap * 4), up((size_t)P * cap);
    for (std::vector<double>* v : {&fields, &s, &up})
      for (double& x : *v)
        if (std::scanf("%lf", &x) != 1) return 2;
    std::vector<int32_t> cell((size_t)P * cap, -1), driven((size_t)P * cap, -1);
    if (with_cell)
      for (int32_t& x : driven)
        if (std::scanf("%d", &x) != 1) return 2;
    const int32_t* pf = with_path_field ? path_field.data() : nullptr;
    auto row = [&](int p, int r) { return &s[((size_t)p * cap + r) * 4]; };
    // forward
    std::vector<double> clearance((size_t)P * cap, fq::no_clearance()), gradient((size_t)P * cap * 4, 0.0);
    std::vector<fq::Nearest> least(P, fq::nearest_none());
    std::vector<int> least_cell(P, -1), n(P);
    for (int p = 0; p < P; ++p) {
      n[p] = fq::live_rows(status[p] > 0, ns[p], cap);
      const int f = fq::grid_of_path(pf, p, G.n_fields);
      for (int r = 0; r < n[p]; ++r) {
        const size_t at = (size_t)p * cap + r;
        double c, g[3];
        int q;
        fq::row_clearance(row(p, r), fields.data(), G, f, outside, true, c, q, g);
        clearance[at] = c, cell[at] = q;
        for (int k = 0; k < 3; ++k) gradient[at * 4 + k] = g[k];
        if (c < least[p].c) least[p].c = c, least[p].index = r, least_cell[p] = q;
      }
    }
    if (!with_cell) driven = cell;
    // backward: one row, one term
    std::vector<double> grad((size_t)P * cap * 4, 0.0);
    for (int p = 0; p < P; ++p) {
      const int f = fq::grid_of_path(pf, p, G.n_fields);
      for (int r = 0; r < n[p]; ++r) {
        const size_t at = (size_t)p * cap + r;
        double gi[3];
        fq::row_gradient(row(p, r), fields.data(), G, f, driven[at], up[at], gi);
        for (int k = 0; k < 3; ++k) grad[at * 4 + k] = gi[k];
      }
    }
    for (int p = 0; p < P; ++p) {
      for (int r = 0; r < cap; ++r) std::printf("%.17g ", clearance[(size_t)p * cap + r]);
      for (int r = 0; r < cap; ++r) std::printf("%d ", cell[(size_t)p * cap + r]);
      for (size_t e = 0; e < (size_t)cap * 4; ++e) std::printf("%.17g ", gradient[(size_t)p * cap * 4 + e]);
      std::printf("%.17g %d %d ", least[p].c, least[p].index, least_cell[p]);
      for (size_t e = 0; e < (size_t)cap * 4; ++e) std::printf("%.17g ", grad[(size_t)p * cap * 4 + e]);
      std::printf("\n");
    }
  }
}

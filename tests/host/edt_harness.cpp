// edt_harness.cpp -- the distance field from an occupancy grid (csrc/mrs_tg_edt.hpp: the ballots of a line and the nearest set bit of
// the x pass, the outward scan of the y and z passes with its two early exits, the tile width, the value at a node) compiled with
// plain g++ for the CPU and driven the way edt_x_kernel, edt_y_kernel and edt_z_kernel drive it: a line as ballots of 64 nodes
// with what the other chunks carry in; ONE array for the transform of the occupancy and of its complement, the node's class in
// the sign bit; a tile of lines copied aside (the kernels' LDS) and scanned, the result written where the input was.
// tests/test_edt_host.py checks it against the brute force of tests/edt_util.py, which knows no passes; tests/test_gpu_edt.py
// checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/edt_harness.cpp -o edt_harness && ./edt_harness < in
//
// Input (whitespace separated), any number of problems until end of input:
//   n_fields nx ny nz flags, hx hy hz z_scale max_distance, occupancy [n_fields][nz][ny][nx] as integers 0 .. 255.
// Every vector has exactly the elements its array has, so a sanitizer build sees every access beyond one.
// Output per grid, one line: fields [nz][ny][nx].  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_edt.hpp"

namespace eq = mrs_tg::edtq;

namespace {

struct Grid {
  int nx, ny, nz, n_fields;
};

// edt_x_kernel: one line
void x_line(const uint8_t* occ, int nx, double wx, bool is_signed, double* fields) {
  const int n_chunks = (nx + eq::kChunk - 1) / eq::kChunk;
  std::vector<uint64_t> m_occ(n_chunks), m_free(n_chunks);
  for (int c = 0; c < n_chunks; ++c) {
    uint64_t m = 0;  // the ballot
    for (int lane = 0; lane < eq::kChunk; ++lane)
      if (c * eq::kChunk + lane < nx && occ[c * eq::kChunk + lane] != 0) m |= 1ull << lane;
    m_occ[c] = m, m_free[c] = ~m & eq::chunk_valid(nx, c);
  }
  for (int c = 0; c < n_chunks; ++c) {
    const int po = eq::chunk_prev(m_occ.data(), c), no = eq::chunk_next(m_occ.data(), n_chunks, c);
    const int pf = eq::chunk_prev(m_free.data(), c), nf = eq::chunk_next(m_free.data(), n_chunks, c);
    for (int lane = 0; lane < eq::kChunk && c * eq::kChunk + lane < nx; ++lane) {
      const bool occupied = (m_occ[c] >> lane) & 1ull;
      const double d = !occupied  ? eq::x_value(eq::x_offset(m_occ[c], c, lane, po, no), wx)
                       : is_signed ? eq::x_value(eq::x_offset(m_free[c], c, lane, pf, nf), wx)
                                   : 0.0;
      fields[c * eq::kChunk + lane] = eq::packed(d, occupied);
    }
  }
}

// the staged tile of the y and z passes: n rows of tx columns at base + l stride + c, c < width
struct Tile {
  size_t base, stride;
  int n, tx, width;
};

void stage(const std::vector<double>& D, const Tile& T, std::vector<double>& tile) {
  tile.assign((size_t)T.n * T.tx, -1.0);  // (a column beyond the width is never read: a negative value would show)
  for (int l = 0; l < T.n; ++l)
    for (int c = 0; c < T.width; ++c) tile[(size_t)l * T.tx + c] = D.at(T.base + (size_t)l * T.stride + c);
}

double scan(const std::vector<double>& tile, const Tile& T, int l, int c, bool occupied, double w, double limit) {
  return eq::scan_line([&](int p) { return eq::seen_by(tile.at((size_t)p * T.tx + c), occupied); }, T.n, l, w, limit);
}

// edt_y_kernel (last = false) and edt_z_kernel (last = true): one tile, in place
void tile_pass(std::vector<double>& fields, const Tile& T, bool last, bool is_signed, double w, double limit, double max_distance,
               std::vector<double>& tile) {
  stage(fields, T, tile);
  for (int l = 0; l < T.n; ++l)
    for (int c = 0; c < T.width; ++c) {
      const size_t at = T.base + (size_t)l * T.stride + c;
      const bool occupied = eq::packed_occupied(tile.at((size_t)l * T.tx + c));
      if (occupied && !is_signed) {
        if (last) fields.at(at) = 0.0;
        continue;
      }
      const double d = scan(tile, T, l, c, occupied, w, limit);
      fields.at(at) = !last ? eq::packed(d, occupied) : (occupied ? eq::occupied_value(d, max_distance) : eq::free_value(d, max_distance));
    }
}

}  // namespace

int main() {
  for (;;) {
    Grid G;
    int flags = 0;
    double h[3], z_scale = 0.0, max_distance = 0.0;
    if (std::scanf("%d", &G.n_fields) != 1) return 0;
    if (std::scanf("%d %d %d %d", &G.nx, &G.ny, &G.nz, &flags) != 4) return 2;
    if (std::scanf("%lf %lf %lf %lf %lf", &h[0], &h[1], &h[2], &z_scale, &max_distance) != 5) return 2;
    if (G.n_fields < 0 || G.nx < 2 || G.ny < 2 || G.nz < 2 || G.nx > eq::kMaxDim || G.ny > eq::kMaxDim || G.nz > eq::kMaxDim) return 2;
    if (!(max_distance > 0.0) || !(z_scale > 0.0) || (flags & ~eq::kSigned) != 0) return 2;
    const size_t slice = (size_t)G.ny * G.nx, grid = slice * G.nz, voxels = grid * G.n_fields;
    if (voxels > 2147483647u) return 2;
    std::vector<uint8_t> occ(voxels);
    for (uint8_t& b : occ) {
      int v;
      if (std::scanf("%d", &v) != 1 || v < 0 || v > 255) return 2;
      b = (uint8_t)v;
    }
    const bool is_signed = (flags & eq::kSigned) != 0;
    const eq::Weights W = eq::weights(h, z_scale);
    const double limit = eq::saturation(max_distance);
    std::vector<double> fields(voxels), tile;
    // x
    for (size_t line = 0; line < voxels / G.nx; ++line) x_line(&occ[line * G.nx], G.nx, W.w[0], is_signed, &fields[line * G.nx]);
    // y, in place through the tile
    {
      const int tx = eq::tile_width(G.ny, G.nx), tiles_x = (G.nx + tx - 1) / tx;
      for (long long b = 0; b < (long long)G.n_fields * G.nz * tiles_x; ++b) {
        const int x0 = (int)(b % tiles_x) * tx;
        const Tile T{(size_t)(b / tiles_x) * slice + x0, (size_t)G.nx, G.ny, tx, G.nx - x0 < tx ? G.nx - x0 : tx};
        tile_pass(fields, T, false, is_signed, W.w[1], limit, max_distance, tile);
      }
    }
    // z and the value at the node
    {
      const int tx = eq::tile_width(G.nz, G.nx), tiles_x = (G.nx + tx - 1) / tx;
      for (long long b = 0; b < (long long)G.n_fields * G.ny * tiles_x; ++b) {
        const int x0 = (int)(b % tiles_x) * tx;
        const long long row = b / tiles_x;
        const Tile T{(size_t)(row / G.ny) * grid + (size_t)(row % G.ny) * G.nx + x0, slice, G.nz, tx, G.nx - x0 < tx ? G.nx - x0 : tx};
        tile_pass(fields, T, true, is_signed, W.w[2], limit, max_distance, tile);
      }
    }
    for (int f = 0; f < G.n_fields; ++f) {
      for (size_t e = 0; e < grid; ++e) std::printf("%.17g ", fields[(size_t)f * grid + e]);
      std::printf("\n");
    }
  }
}

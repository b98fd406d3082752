// edt_region_harness.cpp -- the distance field brought up to date after the occupancy changed inside a box
// (csrc/mrs_tg_edt_region.hpp: reach, core, window, the plan; csrc/mrs_tg_edt.hpp: the per-line routines) compiled with plain g++
// for the CPU and driven the way edt_region_x_kernel, edt_region_y_kernel and edt_region_z_kernel drive it: the x pass on the
// lines of the WINDOW, read from the occupancy at the big grid's strides, its columns of the core kept in a dense workspace
// [W_z][W_y][C_x]; the y pass in place in the workspace through a staged tile, the rows of the core written; the z pass from a
// staged tile of the workspace into the FIELD, the slices of the core alone.  With whole_grid the product runs the full
// transform on that grid in place; here the same windowed passes run with window = core = grid through a workspace of the
// grid's size, which is that transform pass by pass.
// tests/test_edt_region_host.py checks it against the brute force of tests/edt_util.py; tests/test_gpu_edt_region.py checks the
// kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/edt_region_harness.cpp -o edt_region_harness && ./edt_region_harness < in
//
// Input (whitespace separated), any number of problems until end of input: a problem of edt_harness.cpp's grammar,
//   n_fields nx ny nz flags, hx hy hz z_scale max_distance, occupancy [n_fields][nz][ny][nx] as integers 0 .. 255 (the NEW one),
// then the region and a sentinel,
//   field lo_x lo_y lo_z hi_x hi_y hi_z sentinel,
// then the field of the OLD occupancy [n_fields][nz][ny][nx].
// Every vector has exactly the elements its array has (the workspace: the plan's workspace_doubles), so a sanitizer build sees
// every access beyond one.
// Output: one line with the plan -- reach[3] core_lo[3] core_hi[3] window_lo[3] window_hi[3] whole_grid workspace_doubles --,
// then per grid one line, the old field after the update, then per grid one line, an array filled with the sentinel after the
// same update (who is written).  Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_edt_region.hpp"

namespace eq = mrs_tg::edtq;

namespace {

// one grid of the stack and the plan's boxes in it (EdtWindow of mrs_tg_edt_region.hip)
struct Window {
  size_t grid_base;
  int nx, ny;
  int w_lo[3], wn[3], c_off[3], cn[3];
};

// edt_region_x_kernel: one line of the window, n nodes from occ; columns [first, end) go to out
void x_line(const std::vector<uint8_t>& occ, size_t base, int n, int first, int end, double wx, bool is_signed,
            std::vector<double>& ws, size_t out) {
  const int n_chunks = (n + eq::kChunk - 1) / eq::kChunk;
  std::vector<uint64_t> m_occ(n_chunks), m_free(n_chunks);
  for (int c = 0; c < n_chunks; ++c) {
    uint64_t m = 0;  // the ballot
    for (int lane = 0; lane < eq::kChunk; ++lane)
      if (c * eq::kChunk + lane < n && occ.at(base + c * eq::kChunk + lane) != 0) m |= 1ull << lane;
    m_occ[c] = m, m_free[c] = ~m & eq::chunk_valid(n, c);
  }
  for (int c = 0; c < n_chunks; ++c) {
    const int po = eq::chunk_prev(m_occ.data(), c), no = eq::chunk_next(m_occ.data(), n_chunks, c);
    const int pf = eq::chunk_prev(m_free.data(), c), nf = eq::chunk_next(m_free.data(), n_chunks, c);
    for (int lane = 0; lane < eq::kChunk; ++lane) {
      const int i = c * eq::kChunk + lane;
      if (i < first || i >= end) continue;
      const bool occupied = (m_occ[c] >> lane) & 1ull;
      const double d = !occupied  ? eq::x_value(eq::x_offset(m_occ[c], c, lane, po, no), wx)
                       : is_signed ? eq::x_value(eq::x_offset(m_free[c], c, lane, pf, nf), wx)
                                   : 0.0;
      ws.at(out + (i - first)) = eq::packed(d, occupied);
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

// tile_node of mrs_tg_edt_dev.hpp: what a pass leaves at `out` for node (l, c) of the staged tile
void node(double& out, const std::vector<double>& tile, const Tile& T, int l, int c, bool last, bool is_signed, double w,
          double limit, double max_distance) {
  const bool occupied = eq::packed_occupied(tile.at((size_t)l * T.tx + c));
  if (occupied && !is_signed) {
    if (last) out = 0.0;
    return;
  }
  const double d = scan(tile, T, l, c, occupied, w, limit);
  out = !last ? eq::packed(d, occupied) : (occupied ? eq::occupied_value(d, max_distance) : eq::free_value(d, max_distance));
}

// the three launches on one array of fields
void update(const std::vector<uint8_t>& occ, const Window& Wd, const eq::Weights& W, double limit, double max_distance,
            bool is_signed, std::vector<double>& ws, std::vector<double>& fields) {
  const int sx = Wd.cn[0];
  std::vector<double> tile;
  // x: the lines of the window
  for (int line = 0; line < Wd.wn[2] * Wd.wn[1]; ++line) {
    const int k = line / Wd.wn[1], j = line - k * Wd.wn[1];
    const size_t base = Wd.grid_base + ((size_t)(Wd.w_lo[2] + k) * Wd.ny + (size_t)(Wd.w_lo[1] + j)) * Wd.nx + Wd.w_lo[0];
    x_line(occ, base, Wd.wn[0], Wd.c_off[0], Wd.c_off[0] + Wd.cn[0], W.w[0], is_signed, ws, (size_t)line * sx);
  }
  const size_t slice = (size_t)Wd.wn[1] * sx, big_slice = (size_t)Wd.ny * Wd.nx;
  // y: in place in the workspace, the rows of the core
  {
    const int tx = eq::tile_width(Wd.wn[1], sx), tiles_x = (sx + tx - 1) / tx;
    for (int b = 0; b < Wd.wn[2] * tiles_x; ++b) {
      const int x0 = (b % tiles_x) * tx, k = b / tiles_x;
      const Tile T{(size_t)k * slice + x0, (size_t)sx, Wd.wn[1], tx, sx - x0 < tx ? sx - x0 : tx};
      stage(ws, T, tile);
      for (int l = Wd.c_off[1]; l < Wd.c_off[1] + Wd.cn[1]; ++l)
        for (int c = 0; c < T.width; ++c)
          node(ws.at(T.base + (size_t)l * T.stride + c), tile, T, l, c, false, is_signed, W.w[1], limit, max_distance);
    }
  }
  // z: from the workspace into the field, the slices of the core
  const int tx = eq::tile_width(Wd.wn[2], sx), tiles_x = (sx + tx - 1) / tx;
  for (int b = 0; b < Wd.cn[1] * tiles_x; ++b) {
    const int x0 = (b % tiles_x) * tx, j = Wd.c_off[1] + b / tiles_x;
    const Tile T{(size_t)j * sx + x0, slice, Wd.wn[2], tx, sx - x0 < tx ? sx - x0 : tx};
    stage(ws, T, tile);
    const size_t out = Wd.grid_base + (size_t)Wd.w_lo[2] * big_slice + (size_t)(Wd.w_lo[1] + j) * Wd.nx +
                       (size_t)(Wd.w_lo[0] + Wd.c_off[0] + x0);
    for (int l = Wd.c_off[2]; l < Wd.c_off[2] + Wd.cn[2]; ++l)
      for (int c = 0; c < T.width; ++c)
        node(fields.at(out + (size_t)l * big_slice + c), tile, T, l, c, true, is_signed, W.w[2], limit, max_distance);
  }
}

}  // namespace

int main() {
  for (;;) {
    int n_fields, dims[3], flags = 0;
    double h[3], z_scale = 0.0, max_distance = 0.0;
    if (std::scanf("%d", &n_fields) != 1) return 0;
    if (std::scanf("%d %d %d %d", &dims[0], &dims[1], &dims[2], &flags) != 4) return 2;
    if (std::scanf("%lf %lf %lf %lf %lf", &h[0], &h[1], &h[2], &z_scale, &max_distance) != 5) return 2;
    if (n_fields < 1) return 2;
    for (int a = 0; a < 3; ++a)
      if (dims[a] < 2 || dims[a] > eq::kMaxDim) return 2;
    if (!(max_distance > 0.0) || !(z_scale > 0.0) || (flags & ~eq::kSigned) != 0) return 2;
    const size_t grid = (size_t)dims[2] * dims[1] * dims[0], voxels = grid * n_fields;
    if (voxels > 2147483647u) return 2;
    std::vector<uint8_t> occ(voxels);
    for (uint8_t& b : occ) {
      int v;
      if (std::scanf("%d", &v) != 1 || v < 0 || v > 255) return 2;
      b = (uint8_t)v;
    }
    int field, lo[3], hi[3];
    double sentinel;
    if (std::scanf("%d %d %d %d %d %d %d %lf", &field, &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &sentinel) != 8) return 2;
    if (field < 0 || field >= n_fields) return 2;
    for (int a = 0; a < 3; ++a)
      if (lo[a] < 0 || lo[a] > hi[a] || hi[a] >= dims[a]) return 2;
    std::vector<double> fields(voxels), marked(voxels, sentinel);
    for (double& v : fields)
      if (std::scanf("%lf", &v) != 1) return 2;

    const bool is_signed = (flags & eq::kSigned) != 0;
    const eq::Weights W = eq::weights(h, z_scale);
    const double limit = eq::saturation(max_distance);
    const eq::RegionPlan P = eq::plan_region(dims, W, limit, lo, hi);
    Window Wd;
    Wd.grid_base = (size_t)field * grid, Wd.nx = dims[0], Wd.ny = dims[1];
    for (int a = 0; a < 3; ++a) {
      Wd.w_lo[a] = P.window_lo[a], Wd.wn[a] = P.window_n(a);
      Wd.c_off[a] = P.core_lo[a] - P.window_lo[a], Wd.cn[a] = P.core_n(a);
    }
    // (whole_grid: core = window = grid, the full transform of that grid)
    std::vector<double> ws(P.whole_grid ? grid : (size_t)P.workspace_doubles);
    update(occ, Wd, W, limit, max_distance, is_signed, ws, fields);
    update(occ, Wd, W, limit, max_distance, is_signed, ws, marked);

    for (int a = 0; a < 3; ++a) std::printf("%d ", P.reach[a]);
    for (int a = 0; a < 3; ++a) std::printf("%d ", P.core_lo[a]);
    for (int a = 0; a < 3; ++a) std::printf("%d ", P.core_hi[a]);
    for (int a = 0; a < 3; ++a) std::printf("%d ", P.window_lo[a]);
    for (int a = 0; a < 3; ++a) std::printf("%d ", P.window_hi[a]);
    std::printf("%d %lld\n", P.whole_grid, P.workspace_doubles);
    for (const std::vector<double>* A : {&fields, &marked})
      for (int f = 0; f < n_fields; ++f) {
        for (size_t e = 0; e < grid; ++e) std::printf("%.17g ", (*A)[(size_t)f * grid + e]);
        std::printf("\n");
      }
  }
}

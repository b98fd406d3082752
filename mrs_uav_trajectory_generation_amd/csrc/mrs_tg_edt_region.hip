// mrs_tg_edt_region.hip -- the distance field brought up to date after the occupancy changed inside a box
// (mrs_tg_field_update_region): the three passes of mrs_tg_edt.hip on a WINDOW of one grid of the stack, through a dense
// workspace, the result written into the field on the CORE alone.  mrs_tg_edt_region.hpp holds reach, core and window and the
// argument why these are the full rebuild's bits; mrs_tg_edt.hpp the per-line routines, used here as they are; DESIGN.md section
// 11m the measurements.  LANES RUN ALONG x IN EVERY PASS.
// The workspace is [W_z][W_y][C_x] doubles, x fastest: packed() values (the class in the sign bit) as the full transform keeps
// them in its output between the passes.
//   edt_region_x_kernel  a wavefront takes a line of the window (W_x nodes, at most kMaxDim) at a time and reads its occupancy
//                        bytes at the big grid's strides: ballots of 64 nodes to LDS, chunk_prev / chunk_next / x_offset /
//                        x_value as in edt_x_kernel, and writes the columns of C_x into the workspace.
//   edt_region_y_kernel  a workgroup stages a tile of the workspace -- W_y rows of tile_width(W_y, C_x) columns -- in LDS, scans
//                        (edtq::scan_line, edtq::seen_by) and writes the rows of C_y where the input was: in place, the tile is
//                        whole in LDS before the first store.  The other rows keep the x pass's values; nobody reads them again.
//   edt_region_z_kernel  stages W_z slices of a row of C_y and writes free_value / occupied_value for the slices of C_z into the
//                        field at the big grid's address.
// No atomics; the occupancy is only read; every core node of the field is written by exactly one thread and no other element
// of the field is written.  Bounds: a window index is formed from i < W_x (or C_x), a row below W_y, a slice below W_z, and the
// plan's boxes lie inside the grid (plan_region clips them), so every occupancy and field address lies inside the one grid
// `field` of the stack, and every workspace address below workspace_doubles.
// When the window is the whole grid (RegionPlan::whole_grid) the launcher runs the full transform on that grid instead.
#include <hip/hip_runtime.h>

#include "mrs_tg_edt_dev.hpp"
#include "mrs_tg_edt_region.hpp"
#include "mrs_tg_launch.h"

namespace mrs_tg {

namespace {

constexpr int kRegionXWaves = 4;  // lines a workgroup of the x pass takes at a time
constexpr int kRegionXThreads = 64 * kRegionXWaves;

}  // namespace

// one grid of the stack and the plan's boxes in it
struct EdtWindow {
  size_t grid_base;  // of grid `field` in the stack, in voxels
  int nx, ny;        // of the big grid (nz plays no part in an address)
  int w_lo[3];       // the window's low corner in the grid
  int wn[3];         // its extents: W_x, W_y, W_z
  int c_off[3];      // the core's low corner in the window
  int cn[3];         // its extents: C_x, C_y, C_z
};

__global__ __launch_bounds__(kRegionXThreads) void edt_region_x_kernel(const uint8_t* __restrict__ occupancy, EdtWindow Wd,
                                                                       double wx, int is_signed,
                                                                       double* __restrict__ workspace) {
  __shared__ uint64_t s_occ[kRegionXWaves][edtq::kMaxChunks], s_free[kRegionXWaves][edtq::kMaxChunks];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = Wd.wn[0];
  const int n_chunks = (n + edtq::kChunk - 1) / edtq::kChunk;
  const int lines = Wd.wn[2] * Wd.wn[1];
  const int first = Wd.c_off[0], end = Wd.c_off[0] + Wd.cn[0];  // the columns the workspace keeps
  // (the loop is uniform over the workgroup: the barriers are met by every wavefront)
  for (int line0 = blockIdx.x * kRegionXWaves; line0 < lines; line0 += gridDim.x * kRegionXWaves) {
    const int line = line0 + wave;
    const bool active = line < lines;
    const int k = line / Wd.wn[1], j = line - k * Wd.wn[1];
    const size_t base = Wd.grid_base + ((size_t)(Wd.w_lo[2] + k) * (size_t)Wd.ny + (size_t)(Wd.w_lo[1] + j)) * (size_t)Wd.nx +
                        (size_t)Wd.w_lo[0];
    for (int c = 0; c < n_chunks; ++c) {
      const int i = c * edtq::kChunk + lane;
      const bool occupied = active && i < n && occupancy[base + (size_t)i] != 0;
      const uint64_t m = __ballot(occupied);
      if (lane == 0) s_occ[wave][c] = m, s_free[wave][c] = ~m & edtq::chunk_valid(n, c);
    }
    __syncthreads();
    if (active) {
      int prev_occ = -1, next_occ = -1, prev_free = -1, next_free = -1;
      if (lane < n_chunks) {
        prev_occ = edtq::chunk_prev(s_occ[wave], lane), next_occ = edtq::chunk_next(s_occ[wave], n_chunks, lane);
        if (is_signed) prev_free = edtq::chunk_prev(s_free[wave], lane), next_free = edtq::chunk_next(s_free[wave], n_chunks, lane);
      }
      const size_t out = (size_t)line * (size_t)Wd.cn[0];
      for (int c = 0; c < n_chunks; ++c) {
        const int i = c * edtq::kChunk + lane;
        const int po = __shfl(prev_occ, c), no = __shfl(next_occ, c), pf = __shfl(prev_free, c), nf = __shfl(next_free, c);
        if (i >= first && i < end) {
          const uint64_t m = s_occ[wave][c];
          const bool occupied = (m >> lane) & 1ull;
          // a node looks for the nearest node of the OTHER class of its line, as far as the window holds it
          const double d = !occupied  ? edtq::x_value(edtq::x_offset(m, c, lane, po, no), wx)
                           : is_signed ? edtq::x_value(edtq::x_offset(s_free[wave][c], c, lane, pf, nf), wx)
                                       : 0.0;
          workspace[out + (size_t)(i - first)] = edtq::packed(d, occupied);
        }
      }
    }
    __syncthreads();  // (the ballots are read until here)
  }
}

__global__ __launch_bounds__(kEdtThreads) void edt_region_y_kernel(double* __restrict__ workspace, EdtWindow Wd, int tx_log2,
                                                                   int tiles_x, int tiles, double wy, double limit,
                                                                   int is_signed) {
  extern __shared__ __attribute__((aligned(16))) double s_tile[];
  const int tx = 1 << tx_log2, sx = Wd.cn[0];
  const size_t slice = (size_t)Wd.wn[1] * (size_t)sx;
  for (int b = blockIdx.x; b < tiles; b += gridDim.x) {
    const int x0 = (b % tiles_x) * tx, k = b / tiles_x;
    Tile T;
    T.base = (size_t)k * slice + (size_t)x0, T.stride = (size_t)sx, T.n = Wd.wn[1];
    T.tx_log2 = tx_log2, T.width = sx - x0 < tx ? sx - x0 : tx;
    stage_tile(workspace, T, s_tile);
    __syncthreads();  // (the tile is whole in LDS before the first value is written over it)
    const int end = (Wd.c_off[1] + Wd.cn[1]) << tx_log2;
    for (int e = (Wd.c_off[1] << tx_log2) + threadIdx.x; e < end; e += kEdtThreads) {  // the rows of C_y
      const int l = e >> tx_log2, c = e & (tx - 1);
      if (c < T.width)
        tile_node<false>(&workspace[T.base + (size_t)l * T.stride + (size_t)c], s_tile, T, l, c, e, wy, limit, 0.0, is_signed != 0);
    }
    __syncthreads();  // (the tile is read until here)
  }
}

__global__ __launch_bounds__(kEdtThreads) void edt_region_z_kernel(const double* __restrict__ workspace, EdtWindow Wd, int tx_log2,
                                                                   int tiles_x, int tiles, double wz, double limit,
                                                                   double max_distance, int is_signed,
                                                                   double* __restrict__ fields) {
  extern __shared__ __attribute__((aligned(16))) double s_tile[];
  const int tx = 1 << tx_log2, sx = Wd.cn[0];
  const size_t slice = (size_t)Wd.wn[1] * (size_t)sx, big_slice = (size_t)Wd.ny * (size_t)Wd.nx;
  for (int b = blockIdx.x; b < tiles; b += gridDim.x) {
    const int x0 = (b % tiles_x) * tx, j = Wd.c_off[1] + b / tiles_x;  // a row of C_y, as a row of the window
    Tile T;
    T.base = (size_t)j * (size_t)sx + (size_t)x0, T.stride = slice, T.n = Wd.wn[2];
    T.tx_log2 = tx_log2, T.width = sx - x0 < tx ? sx - x0 : tx;
    stage_tile(workspace, T, s_tile);
    __syncthreads();
    // node (l, c) of the tile in the field: slice w_lo z + l, row w_lo y + j, column w_lo x + c_off x + x0 + c
    const size_t out = Wd.grid_base + (size_t)Wd.w_lo[2] * big_slice + (size_t)(Wd.w_lo[1] + j) * (size_t)Wd.nx +
                       (size_t)(Wd.w_lo[0] + Wd.c_off[0] + x0);
    const int end = (Wd.c_off[2] + Wd.cn[2]) << tx_log2;
    for (int e = (Wd.c_off[2] << tx_log2) + threadIdx.x; e < end; e += kEdtThreads) {  // the slices of C_z
      const int l = e >> tx_log2, c = e & (tx - 1);
      if (c < T.width)
        tile_node<true>(&fields[out + (size_t)l * big_slice + (size_t)c], s_tile, T, l, c, e, wz, limit, max_distance, is_signed != 0);
    }
    __syncthreads();  // (the tile is read until here)
  }
}

hipError_t launch_field_update_region(const uint8_t* occupancy, const int (&dims)[3], int field, const edtq::RegionPlan& P,
                                      const edtq::Weights& W, double limit, double max_distance, bool is_signed, double* workspace,
                                      double* fields, hipStream_t stream) {
  const size_t grid = (size_t)dims[2] * (size_t)dims[1] * (size_t)dims[0];
  if (P.whole_grid)  // (takes the pending timer itself)
    return launch_field_from_occupancy(occupancy + (size_t)field * grid, dims, 1, W, limit, max_distance, is_signed,
                                       fields + (size_t)field * grid, stream);
  const KernelTimer kt = take_kernel_timer();  // the family: edt_region_x_kernel's start to edt_region_z_kernel's end
  EdtWindow Wd;
  Wd.grid_base = (size_t)field * grid, Wd.nx = dims[0], Wd.ny = dims[1];
  for (int a = 0; a < 3; ++a) {
    Wd.w_lo[a] = P.window_lo[a], Wd.wn[a] = P.window_n(a);
    Wd.c_off[a] = P.core_lo[a] - P.window_lo[a], Wd.cn[a] = P.core_n(a);
  }
  const int sign = is_signed ? 1 : 0;
  const int sx = Wd.cn[0];
  const long long lines = (long long)Wd.wn[2] * Wd.wn[1];  // (at most kMaxDim^2)
  MRS_TG_LAUNCH_EXT(edt_region_x_kernel, dim3(edt_blocks_for((lines + kRegionXWaves - 1) / kRegionXWaves)), dim3(kRegionXThreads), 0,
                    stream, kt.start, nullptr, 0, occupancy, Wd, W.w[0], sign, workspace);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  {
    const int tx = edtq::tile_width(Wd.wn[1], sx), tiles_x = (sx + tx - 1) / tx;
    const long long tiles = (long long)Wd.wn[2] * tiles_x;
    const size_t lds = (size_t)Wd.wn[1] * (size_t)tx * sizeof(double);
    if (hipError_t e = prepare_dynamic_lds(MRS_TG_KERNEL(edt_region_y_kernel), lds); e != hipSuccess) return e;
    MRS_TG_LAUNCH_EXT(edt_region_y_kernel, dim3(edt_blocks_for(tiles)), dim3(kEdtThreads), lds, stream, nullptr, nullptr, 0, workspace,
                      Wd, edt_log2_of(tx), tiles_x, (int)tiles, W.w[1], limit, sign);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  const int tx = edtq::tile_width(Wd.wn[2], sx), tiles_x = (sx + tx - 1) / tx;
  const long long tiles = (long long)Wd.cn[1] * tiles_x;
  const size_t lds = (size_t)Wd.wn[2] * (size_t)tx * sizeof(double);
  if (hipError_t e = prepare_dynamic_lds(MRS_TG_KERNEL(edt_region_z_kernel), lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_EXT(edt_region_z_kernel, dim3(edt_blocks_for(tiles)), dim3(kEdtThreads), lds, stream, nullptr, kt.stop, 0,
                    (const double*)workspace, Wd, edt_log2_of(tx), tiles_x, (int)tiles, W.w[2], limit, max_distance, sign, fields);
  return hipGetLastError();
}

}  // namespace mrs_tg

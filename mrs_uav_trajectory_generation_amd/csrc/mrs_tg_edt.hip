// mrs_tg_edt.hip -- the voxel grid of (signed) distances from an occupancy grid, by an exact Euclidean distance transform in three
// passes (mrs_tg_field_from_occupancy); mrs_tg_edt.hpp holds the definition, the per-line routines and the arguments why no bit
// moves, DESIGN.md section 11l the measurements.  LANES RUN ALONG x IN EVERY PASS, so every load and store of a wavefront is a
// contiguous run.
// ONE ARRAY, the output, holds the transform of the occupancy AND that of its complement between the passes, the node's class in
// the sign bit (edtq::packed; the header says why the two never need the same element): no workspace, and the y and z passes
// never read the occupancy.
//   edt_x_kernel  a wavefront takes a line of nx bytes at a time.  One ballot of the occupancy per chunk of 64 nodes; the ballots of
//                 the line (and of its complement, which the signed field needs) go to LDS, at most kMaxChunks each.  Lane c looks
//                 up what chunk c is handed from the chunks in front of and behind it (edtq::chunk_prev / chunk_next); then every
//                 node takes the nearest node of the OTHER class at or below and at or above its lane from clz / ctz on the masked
//                 ballot (edtq::x_offset) and writes wx d^2 (edtq::x_value), +inf where the line has none, negated where the node
//                 is occupied.  No scan.
//   edt_y_kernel  a workgroup stages a tile of lines along y -- ny rows of tile_width(ny, nx) doubles, rows of the tile contiguous in
//                 memory -- in LDS, then every thread scans outward along its node's line in LDS (edtq::scan_line), a node of its
//                 own class showing its partial distance and a node of the other class being a source at 0 (edtq::seen_by), and
//                 writes the result where the input was: in place, the tile belongs to this workgroup alone and is whole in LDS
//                 before the first store.
//   edt_z_kernel  the same along z, and the last pass: a free node takes min(sqrt(D_occ), max_distance); an occupied node 0.0 or,
//                 in a signed field, -min(sqrt(D_free), max_distance).
// The passes loop over their lines or tiles by the grid's stride, so that a launch never has more than kEdtBlocks workgroups.
// No atomics; the occupancy is only read; every output element is written by exactly one thread in every pass (an occupied node
// of an unsigned field is left as it is by the y pass).  Bounds: a node
// index is formed only from i < nx, l < n and a line or tile index below its count, so every address lies in [0, voxels).
#include <hip/hip_runtime.h>

#include "mrs_tg_edt_dev.hpp"
#include "mrs_tg_launch.h"

namespace mrs_tg {

namespace {

constexpr int kEdtXWaves = 4;                  // lines a workgroup of the x pass takes at a time
constexpr int kEdtXThreads = 64 * kEdtXWaves;

}  // namespace

struct EdtGrid {
  int nx, ny, nz, n_fields;
};

// (Tile, stage_tile, scan_tile, tile_node: mrs_tg_edt_dev.hpp, shared with the update of a changed box)

namespace {

// One pass along y (Last = false) or z (Last = true) over the tiles of this workgroup, in place.  An occupied node of an
// unsigned field keeps its -0.0 through the y pass and becomes 0.0 in the last.
template <bool Last>
__device__ inline void axis_pass(double* fields, const EdtGrid& G, int tx_log2, int tiles_x, long long tiles, double w,
                                 double limit, double max_distance, bool is_signed, double* __restrict__ s_tile) {
  const int tx = 1 << tx_log2;
  const size_t slice = (size_t)G.ny * (size_t)G.nx;
  for (long long b = blockIdx.x; b < tiles; b += gridDim.x) {
    const int x0 = (int)(b % tiles_x) * tx;
    const long long outer = b / tiles_x;  // y: the slice f nz + k;  z: the row f ny + j
    Tile T;
    if (Last) {
      T.base = (size_t)(outer / G.ny) * (size_t)G.nz * slice + (size_t)(outer % G.ny) * (size_t)G.nx + (size_t)x0;
      T.stride = slice, T.n = G.nz;
    } else {
      T.base = (size_t)outer * slice + (size_t)x0;
      T.stride = (size_t)G.nx, T.n = G.ny;
    }
    T.tx_log2 = tx_log2, T.width = G.nx - x0 < tx ? G.nx - x0 : tx;
    stage_tile(fields, T, s_tile);
    __syncthreads();  // (the tile is whole in LDS before the first value is written over it)
    const int total = T.n << tx_log2;
    for (int e = threadIdx.x; e < total; e += kEdtThreads) {
      const int l = e >> tx_log2, c = e & (tx - 1);
      if (c < T.width) {
        const size_t at = T.base + (size_t)l * T.stride + (size_t)c;
        tile_node<Last>(&fields[at], s_tile, T, l, c, e, w, limit, max_distance, is_signed);
      }
    }
    __syncthreads();  // (the tile is read until here)
  }
}

}  // namespace

__global__ __launch_bounds__(kEdtXThreads) void edt_x_kernel(const uint8_t* __restrict__ occupancy, int nx, long long lines,
                                                             double wx, int is_signed, double* __restrict__ fields) {
  __shared__ uint64_t s_occ[kEdtXWaves][edtq::kMaxChunks], s_free[kEdtXWaves][edtq::kMaxChunks];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n_chunks = (nx + edtq::kChunk - 1) / edtq::kChunk;
  // (the loop is uniform over the workgroup: the barriers are met by every wavefront)
  for (long long line0 = (long long)blockIdx.x * kEdtXWaves; line0 < lines; line0 += (long long)gridDim.x * kEdtXWaves) {
    const long long line = line0 + wave;
    const bool active = line < lines;
    const size_t base = (size_t)line * (size_t)nx;
    for (int c = 0; c < n_chunks; ++c) {
      const int i = c * edtq::kChunk + lane;
      const bool occupied = active && i < nx && occupancy[base + (size_t)i] != 0;
      const uint64_t m = __ballot(occupied);
      if (lane == 0) s_occ[wave][c] = m, s_free[wave][c] = ~m & edtq::chunk_valid(nx, c);
    }
    __syncthreads();
    if (active) {
      int prev_occ = -1, next_occ = -1, prev_free = -1, next_free = -1;
      if (lane < n_chunks) {
        prev_occ = edtq::chunk_prev(s_occ[wave], lane), next_occ = edtq::chunk_next(s_occ[wave], n_chunks, lane);
        if (is_signed) prev_free = edtq::chunk_prev(s_free[wave], lane), next_free = edtq::chunk_next(s_free[wave], n_chunks, lane);
      }
      for (int c = 0; c < n_chunks; ++c) {
        const int i = c * edtq::kChunk + lane;
        const int po = __shfl(prev_occ, c), no = __shfl(next_occ, c), pf = __shfl(prev_free, c), nf = __shfl(next_free, c);
        if (i < nx) {
          const uint64_t m = s_occ[wave][c];
          const bool occupied = (m >> lane) & 1ull;
          // a node looks for the nearest node of the OTHER class of its line
          const double d = !occupied  ? edtq::x_value(edtq::x_offset(m, c, lane, po, no), wx)
                           : is_signed ? edtq::x_value(edtq::x_offset(s_free[wave][c], c, lane, pf, nf), wx)
                                       : 0.0;
          fields[base + (size_t)i] = edtq::packed(d, occupied);
        }
      }
    }
    __syncthreads();  // (the ballots are read until here)
  }
}

__global__ __launch_bounds__(kEdtThreads) void edt_y_kernel(double* __restrict__ fields, EdtGrid G, int tx_log2, int tiles_x,
                                                            long long tiles, double wy, double limit, int is_signed) {
  extern __shared__ __attribute__((aligned(16))) double s_tile[];
  axis_pass<false>(fields, G, tx_log2, tiles_x, tiles, wy, limit, 0.0, is_signed != 0, s_tile);
}

__global__ __launch_bounds__(kEdtThreads) void edt_z_kernel(double* __restrict__ fields, EdtGrid G, int tx_log2, int tiles_x,
                                                            long long tiles, double wz, double limit, double max_distance,
                                                            int is_signed) {
  extern __shared__ __attribute__((aligned(16))) double s_tile[];
  axis_pass<true>(fields, G, tx_log2, tiles_x, tiles, wz, limit, max_distance, is_signed != 0, s_tile);
}

hipError_t launch_field_from_occupancy(const uint8_t* occupancy, const int (&dims)[3], int n_fields, const edtq::Weights& W,
                                       double limit, double max_distance, bool is_signed, double* fields, hipStream_t stream) {
  const KernelTimer kt = take_kernel_timer();  // the family: edt_x_kernel's start to edt_z_kernel's end
  if (n_fields == 0) return hipSuccess;
  const EdtGrid G{dims[0], dims[1], dims[2], n_fields};
  const int sign = is_signed ? 1 : 0;
  const long long lines = (long long)n_fields * G.nz * G.ny;
  MRS_TG_LAUNCH_EXT(edt_x_kernel, dim3(edt_blocks_for((lines + kEdtXWaves - 1) / kEdtXWaves)), dim3(kEdtXThreads), 0, stream, kt.start,
                    nullptr, 0, occupancy, G.nx, lines, W.w[0], sign, fields);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  {
    const int tx = edtq::tile_width(G.ny, G.nx), tiles_x = (G.nx + tx - 1) / tx;
    const long long tiles = (long long)n_fields * G.nz * tiles_x;
    const size_t lds = (size_t)G.ny * (size_t)tx * sizeof(double);
    if (hipError_t e = prepare_dynamic_lds(MRS_TG_KERNEL(edt_y_kernel), lds); e != hipSuccess) return e;
    MRS_TG_LAUNCH_EXT(edt_y_kernel, dim3(edt_blocks_for(tiles)), dim3(kEdtThreads), lds, stream, nullptr, nullptr, 0, fields, G,
                      edt_log2_of(tx), tiles_x, tiles, W.w[1], limit, sign);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  const int tx = edtq::tile_width(G.nz, G.nx), tiles_x = (G.nx + tx - 1) / tx;
  const long long tiles = (long long)n_fields * G.ny * tiles_x;
  const size_t lds = (size_t)G.nz * (size_t)tx * sizeof(double);
  if (hipError_t e = prepare_dynamic_lds(MRS_TG_KERNEL(edt_z_kernel), lds); e != hipSuccess) return e;
  MRS_TG_LAUNCH_EXT(edt_z_kernel, dim3(edt_blocks_for(tiles)), dim3(kEdtThreads), lds, stream, nullptr, kt.stop, 0, fields, G,
                    edt_log2_of(tx), tiles_x, tiles, W.w[2], limit, max_distance, sign);
  return hipGetLastError();
}

}  // namespace mrs_tg

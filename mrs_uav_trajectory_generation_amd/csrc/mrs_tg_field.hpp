// mrs_tg_field.hpp -- the clearance of every row from a static map given as a VOXEL GRID OF SIGNED DISTANCES (an ESDF), looked up
// by trilinear interpolation (mrs_tg_plan_field_clearance, field_clearance_kernel), and its backward pass
// (mrs_tg_plan_field_clearance_vjp, field_clearance_vjp_kernel); DESIGN.md section 11k.  Where mrs_tg_obstacle.hpp walks a list of
// obstacles per row, this reads eight voxels per row whatever the size of the map: the spatial index over a static map, built
// once ("a field from a list of obstacles").
//
// fields [n_fields][nz][ny][nx] doubles, x fastest: grids of ONE geometry stacked in one array.  The value with indices
// (i, j, k) sits at origin + (i hx, j hy, k hz): the grid is node-centred.  path_field [n_paths] names the grid a path sees
// (null: grid 0); an entry outside [0, n_fields) means the path sees none.  For a live row (x, y, z, .) of a path that sees grid
// f, in this order and with no product contracted into a fused multiply-add:
//   ux = (x - ox) / hx   (a true division; uy, uz alike)
//   INSIDE  <=>  0 <= u && u <= n - 1 on every axis, tested in double: a NaN fails, a huge u is never converted to an integer
//   i = (int)ux, lowered to nx - 2 when above it (the upper face belongs to the last cell, with tx = 1);  tx = ux - (double)i
//   lerp(a, b, t) = a + t (b - a);  fIJK the voxel at (i + I, j + J, k + K)
//   c00 = lerp(f000, f100, tx)  c10 = lerp(f010, f110, tx)  c01 = lerp(f001, f101, tx)  c11 = lerp(f011, f111, tx)
//   c0 = lerp(c00, c10, ty)  c1 = lerp(c01, c11, ty)  clearance = lerp(c0, c1, tz)
// and the field's gradient at the row, differences first and lerps afterwards:
//   gx = lerp(lerp(f100 - f000, f110 - f010, ty), lerp(f101 - f001, f111 - f011, ty), tz) / hx
//   gy = lerp(lerp(f010 - f000, f110 - f100, tx), lerp(f011 - f001, f111 - f101, tx), tz) / hy
//   gz = lerp(lerp(f001 - f000, f101 - f100, tx), lerp(f011 - f010, f111 - f110, tx), ty) / hz
// cell = ((f nz + k) ny + j) nx + i, the low corner's index in the WHOLE fields array (an int32: the ABI refuses a larger array).
// A live row that is not inside gets the caller's outside_value with cell = -1; a path that sees no grid gets +inf / -1.  Voxel
// values are ordinary data: an infinite or NaN voxel gives what the arithmetic makes of it, and a NaN clearance never becomes
// a minimum (clrq::better's order).  Plain double, __host__ __device__, on mrs_tg_hd.hpp alone (through mrs_tg_clearance.hpp,
// whose tie rule, neutral value and live rows are used as they are): tests/host/field_harness.cpp runs this file under g++.
//
// Backward, the cell held fixed (as `nearest` is in mrs_tg_obstacle.hpp).  With g = dL/dclearance of a row and its recorded cell,
//   dL/drow = (g gx, g gy, g gz)           row_gradient
// with gx, gy, gz recomputed from the row and the cell: t = u - (double)i is NOT clamped again, so for the forward's own cells
// g * gradient_out and the backward's output are the same bits.  Exactly 0 come from g == 0 (so the +inf rows never make a NaN),
// cell = -1, a cell that decodes to a grid other than the path's own, and a cell that decodes to i, j, k outside [0, n - 2]
// (cell_of_path) -- none of which dereferences a voxel.  A cell that passes has all eight corners inside the path's own grid.
//
// Out of scope.  float32 fields.  A gradient with respect to the field (a static map).  No gradient flows through the choice
// of the cell.  Interpolation smoother than trilinear (the gradient jumps across cell faces).  Splitting one path over several
// workgroups.  (Building the field is not this file's business: mrs_tg_edt.hpp does it from an occupancy grid, the recipe of
// DESIGN.md section 11k from a list of obstacles.)
#pragma once

#include "mrs_tg_clearance.hpp"
#include "mrs_tg_hd.hpp"

namespace mrs_tg {
namespace fldq {

using clrq::better;
using clrq::live_rows;
using clrq::Nearest;
using clrq::nearest_none;
using clrq::no_clearance;

// the geometry all grids of one fields array share (mrs_tg_field_geometry, checked by the ABI: n >= 2, h finite and positive,
// o finite, n_fields nz ny nx <= 2^31 - 1)
struct Geometry {
  double o[3], h[3];
  int n[3];  // nx, ny, nz
  int n_fields;
};

// the grid path p sees, -1 for none: path_field (null: grid 0) outside [0, n_fields).  Reads path_field[p] only.
MRS_TG_HD inline int grid_of_path(const int32_t* path_field, int p, int n_fields) {
  MRS_TG_NO_CONTRACT
  const int f = path_field ? path_field[p] : 0;
  return (f < 0 || f >= n_fields) ? -1 : f;
}

// u of a coordinate, and of a row
MRS_TG_HD inline double grid_coordinate(double x, double o, double h) {
  MRS_TG_NO_CONTRACT
  return (x - o) / h;
}

// the inside test and the cell choice along one axis: false where u is outside [0, n - 1] or not a number (i, t untouched)
MRS_TG_HD inline bool axis_cell(double u, int n, int& i, double& t) {
  MRS_TG_NO_CONTRACT
  if (!(0.0 <= u && u <= (double)(n - 1))) return false;
  int c = (int)u;  // (0 <= u <= n - 1 < 2^31: the conversion is defined)
  if (c > n - 2) c = n - 2;
  i = c, t = u - (double)c;
  return true;
}

// cell encode (64-bit on the way: the product is below 2^31 by the ABI's check)
MRS_TG_HD inline int encode_cell(const Geometry& G, int f, int i, int j, int k) {
  MRS_TG_NO_CONTRACT
  return (int)((((long long)f * G.n[2] + k) * G.n[1] + j) * G.n[0] + i);
}
// ... and decode: any non-negative cell gives i in [0, nx), j in [0, ny), k in [0, nz) and an f >= 0
MRS_TG_HD inline void decode_cell(const Geometry& G, int cell, int& f, int& i, int& j, int& k) {
  MRS_TG_NO_CONTRACT
  int r = cell;
  i = r % G.n[0], r /= G.n[0];
  j = r % G.n[1], r /= G.n[1];
  k = r % G.n[2], f = r / G.n[2];
}
// Whether a recorded cell is a low corner in the grid f (>= 0) of its path: only then is a voxel dereferenced, and then all
// eight corners lie inside grid f, so inside the fields array.
MRS_TG_HD inline bool cell_of_path(const Geometry& G, int f, int cell, int& i, int& j, int& k) {
  MRS_TG_NO_CONTRACT
  if (cell < 0 || f < 0) return false;
  int cf;
  decode_cell(G, cell, cf, i, j, k);
  return cf == f && i <= G.n[0] - 2 && j <= G.n[1] - 2 && k <= G.n[2] - 2;
}

// the row's cell in grid f (>= 0) and its three t; false (nothing written) where the row is not inside
MRS_TG_HD inline bool locate(const double* row, const Geometry& G, int f, int& cell, double (&t)[3]) {
  MRS_TG_NO_CONTRACT
  int c[3];
  double tt[3];
  bool inside = true;
  MRS_TG_UNROLL
  for (int a = 0; a < 3; ++a) inside = axis_cell(grid_coordinate(row[a], G.o[a], G.h[a]), G.n[a], c[a], tt[a]) && inside;
  if (!inside) return false;
  cell = encode_cell(G, f, c[0], c[1], c[2]);
  t[0] = tt[0], t[1] = tt[1], t[2] = tt[2];
  return true;
}

// the eight corners of a cell: v[I + 2 J + 4 K] = the voxel at (i + I, j + J, k + K)
MRS_TG_HD inline void load_corners(const double* fields, const Geometry& G, int cell, double (&v)[8]) {
  MRS_TG_NO_CONTRACT
  const size_t sy = (size_t)G.n[0], sz = (size_t)G.n[0] * (size_t)G.n[1];
  const double* base = fields + (size_t)cell;
  v[0] = base[0], v[1] = base[1], v[2] = base[sy], v[3] = base[sy + 1];
  v[4] = base[sz], v[5] = base[sz + 1], v[6] = base[sz + sy], v[7] = base[sz + sy + 1];
}

MRS_TG_HD inline double lerp(double a, double b, double t) {
  MRS_TG_NO_CONTRACT
  return a + t * (b - a);
}

// the interpolant: four lerps in x, two in y, one in z
MRS_TG_HD inline double interpolate(const double (&v)[8], const double (&t)[3]) {
  MRS_TG_NO_CONTRACT
  const double c00 = lerp(v[0], v[1], t[0]), c10 = lerp(v[2], v[3], t[0]);
  const double c01 = lerp(v[4], v[5], t[0]), c11 = lerp(v[6], v[7], t[0]);
  const double c0 = lerp(c00, c10, t[1]), c1 = lerp(c01, c11, t[1]);
  return lerp(c0, c1, t[2]);
}

// the field's gradient at the row: differences first, lerps afterwards, the spacing last
MRS_TG_HD inline void gradient(const double (&v)[8], const double (&t)[3], const Geometry& G, double (&g)[3]) {
  MRS_TG_NO_CONTRACT
  g[0] = lerp(lerp(v[1] - v[0], v[3] - v[2], t[1]), lerp(v[5] - v[4], v[7] - v[6], t[1]), t[2]) / G.h[0];
  g[1] = lerp(lerp(v[2] - v[0], v[3] - v[1], t[0]), lerp(v[6] - v[4], v[7] - v[5], t[0]), t[2]) / G.h[1];
  g[2] = lerp(lerp(v[4] - v[0], v[5] - v[1], t[0]), lerp(v[6] - v[2], v[7] - v[3], t[0]), t[1]) / G.h[2];
}

// the t of a row against a FIXED low corner (i, j, k): not clamped, not tested
MRS_TG_HD inline void offsets_in_cell(const double* row, const Geometry& G, int i, int j, int k, double (&t)[3]) {
  MRS_TG_NO_CONTRACT
  t[0] = grid_coordinate(row[0], G.o[0], G.h[0]) - (double)i;
  t[1] = grid_coordinate(row[1], G.o[1], G.h[1]) - (double)j;
  t[2] = grid_coordinate(row[2], G.o[2], G.h[2]) - (double)k;
}

// What the forward gives a live row of a path that sees grid f (-1: none): clearance, cell and, with want_gradient, the field's
// gradient (zeros wherever cell = -1).  The definition; the kernel issues the same calls with its loads hoisted.
MRS_TG_HD inline void row_clearance(const double* row, const double* fields, const Geometry& G, int f, double outside_value,
                                    bool want_gradient, double& clearance, int& cell, double (&g)[3]) {
  MRS_TG_NO_CONTRACT
  g[0] = g[1] = g[2] = 0.0;
  cell = -1;
  if (f < 0) {
    clearance = no_clearance();
    return;
  }
  double t[3];
  if (!locate(row, G, f, cell, t)) {
    clearance = outside_value;
    return;
  }
  double v[8];
  load_corners(fields, G, cell, v);
  clearance = interpolate(v, t);
  if (want_gradient) gradient(v, t, G, g);
}

// dL/drow of a live row from its upstream g and its recorded cell: what field_clearance_vjp_kernel writes (with a 0 behind)
MRS_TG_HD inline void row_gradient(const double* row, const double* fields, const Geometry& G, int f, int cell, double g,
                                   double (&gi)[3]) {
  MRS_TG_NO_CONTRACT
  gi[0] = gi[1] = gi[2] = 0.0;
  int i, j, k;
  if (g == 0.0 || !cell_of_path(G, f, cell, i, j, k)) return;
  double t[3], v[8], d[3];
  offsets_in_cell(row, G, i, j, k, t);
  load_corners(fields, G, cell, v);
  gradient(v, t, G, d);
  gi[0] = g * d[0], gi[1] = g * d[1], gi[2] = g * d[2];
}

}  // namespace fldq
}  // namespace mrs_tg

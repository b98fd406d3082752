// mrs_tg_edt_region.hpp -- the distance field of mrs_tg_edt.hpp brought up to date after the occupancy changed inside a BOX
// (mrs_tg_field_update_region; edt_region_x_kernel, edt_region_y_kernel, edt_region_z_kernel in mrs_tg_edt_region.hip); DESIGN.md
// section 11m.  A mapping stack rewrites a small box of voxels per scan; the field of the new occupancy differs from the old
// one only near that box, because the cap max_distance bounds how far a voxel is felt.  This header says how far, which nodes
// are recomputed, from which occupancy, and why the result is the full rebuild's in every bit.
//
// Reach.  T = edtq::saturation(max_distance), w_a the weight of axis a (edtq::weights), n_a its dim.  The reach rho_a is the
// largest integer d >= 0 with w_a (double)(d d) < T, held to n_a - 1; it IS n_a - 1 when T = +inf.  w (double)(d d) does not
// decrease with d, so w_a (double)(d d) >= T for every d > rho_a that the axis has, and offset rho_a + 1 is exactly where
// scan_line stops on t >= limit (where the axis has such an offset at all).
//
// Boxes, inclusive node indices, each clipped to the grid.  B = [lo, hi] holds every voxel whose occupancy byte may differ
// between the old map and the new.
//   core    C = B grown by rho_a on either side of axis a      the only nodes whose value can differ from the old field
//   window  W = C grown by rho_a on either side of axis a      the only occupancy the new values on C depend on
//
// (1) A node v outside C keeps its bits.  v lies outside B, so its class is the same in both maps.  There is an axis a on
// which v is more than rho_a away from every voxel of B (else v were in C), so a candidate q = fl(fl(wx di^2 + wy dj^2) + wz
// dk^2) between v and a voxel u of B has the term w_a (double)(d_a d_a) >= T; every term is >= 0 and fl(. + .) is monotone, so
// q >= T.  The candidates of v's minimum that do not involve B are the same doubles in both maps.  If the old D(v) < T it is
// attained at an unchanged voxel, which is a candidate of the new minimum too, and no new candidate is below T unless it is an
// old one: new D = old D.  If the old D(v) >= T, a new D < T would be attained at an unchanged voxel and be an old candidate:
// so new D >= T.  rt(D) = max_distance for every D >= T (mrs_tg_edt.hpp), so the value is the same double either way; an
// occupied node of an unsigned field holds 0.0 in both.
//
// (2) The three passes on W alone, nodes outside W treated as non-existent, give on C values D3' with "D3' == D3 where D3 < T,
// D3' >= T where D3 >= T" (D3 the definition's minimum over the whole grid), which is the property mrs_tg_edt.hpp's saturation
// claim carries from pass to pass.
//   x  For x in C_x: if D1 < T the nearest node of the other class in the line is at an offset d with wx (double)(d d) < T, so
//      d <= rho_x and the node lies in W_x: the windowed nearest node is the same one, D1' == D1.  If D1 >= T the windowed
//      minimum runs over fewer nodes: D1' >= D1 >= T (+inf where the window's line has none).
//   y  scan_line stops at the first offset d with wy (double)(d d) >= T, that is at rho_y + 1, so from a row in C_y it looks at
//      rows within rho_y: all in W_y or outside the grid, where the full transform's scan finds nothing either.  The windowed
//      scan therefore sees the candidates of the full transform's (shortened) scan, from inputs with the property: by the
//      header's claim its output has the property.  Needed of the x pass: columns C_x, rows W_y.
//   z  the same with rho_z, from slices C_z looking into W_z.  Needed of the y pass: columns C_x, rows C_y, slices W_z.
// rt maps both D3 and D3' to the same double (equal below T, max_distance from T on), and the full rebuild, whose scans are
// shortened in the same way, does the same: the update leaves the full rebuild's bits on C, and by (1) everywhere.
//
// The workspace holds what the separable dependency needs and no more: columns C_x (the x pass reads the occupancy of W_x
// but keeps D1 on C_x alone), rows W_y, slices W_z -- [W_z][W_y][C_x] doubles, x fastest, packed() values as in the full
// transform.  The y pass writes rows C_y only, the z pass reads rows C_y and writes slices C_z of the field.  RegionPlan::
// workspace_doubles is the contract.
//
// whole_grid: W is the whole grid on every axis (always so with max_distance = +inf).  Nothing is saved by a window then, and
// the caller of plan_region runs the full transform on that one grid, in place, without a workspace (workspace_doubles = 0).
// That transform writes every node of the grid, so the plan then reports the whole grid as its core: "the core is what is
// written, and holds every node that can change" is true on both routes (by (1) the nodes added to it get their old bits).
//
// Plain double and int, __host__ __device__, on mrs_tg_hd.hpp and mrs_tg_edt.hpp alone: tests/host/edt_region_harness.cpp runs
// this under g++.
#pragma once

#include "mrs_tg_edt.hpp"

namespace mrs_tg {
namespace edtq {

// rho of the header comment for an axis of n nodes with weight w
MRS_TG_HD inline int reach(double w, double T, int n) {
  MRS_TG_NO_CONTRACT
  if (!(T < infinity())) return n - 1;
  int d = 0;
  while (d < n - 1 && w * (double)((d + 1) * (d + 1)) < T) ++d;
  return d;
}

struct RegionPlan {
  int reach[3];
  int core_lo[3], core_hi[3];      // C, inclusive, x y z
  int window_lo[3], window_hi[3];  // W
  int whole_grid;                  // W is the grid on every axis: the full transform of that grid, no workspace
  long long workspace_doubles;     // [W_z][W_y][C_x], 0 with whole_grid

  MRS_TG_HD int core_n(int a) const { return core_hi[a] - core_lo[a] + 1; }
  MRS_TG_HD int window_n(int a) const { return window_hi[a] - window_lo[a] + 1; }
  MRS_TG_HD long long window_voxels() const { return (long long)window_n(0) * window_n(1) * window_n(2); }
};

// dims = nx, ny, nz; 0 <= lo[a] <= hi[a] < dims[a] (the caller's check)
inline RegionPlan plan_region(const int (&dims)[3], const Weights& W, double T, const int (&lo)[3], const int (&hi)[3]) {
  MRS_TG_NO_CONTRACT
  RegionPlan P;
  P.whole_grid = 1;
  for (int a = 0; a < 3; ++a) {
    const int r = reach(W.w[a], T, dims[a]), last = dims[a] - 1;
    P.reach[a] = r;
    P.core_lo[a] = lo[a] - r > 0 ? lo[a] - r : 0;
    P.core_hi[a] = hi[a] < last - r ? hi[a] + r : last;  // (no sum beyond an int: r <= last)
    P.window_lo[a] = P.core_lo[a] - r > 0 ? P.core_lo[a] - r : 0;
    P.window_hi[a] = P.core_hi[a] < last - r ? P.core_hi[a] + r : last;
    if (P.window_lo[a] != 0 || P.window_hi[a] != last) P.whole_grid = 0;
  }
  if (P.whole_grid)  // the full transform writes every node of the grid: the plan says so
    for (int a = 0; a < 3; ++a) P.core_lo[a] = 0, P.core_hi[a] = dims[a] - 1;
  P.workspace_doubles = P.whole_grid ? 0 : (long long)P.window_n(2) * P.window_n(1) * P.core_n(0);
  return P;
}

}  // namespace edtq
}  // namespace mrs_tg

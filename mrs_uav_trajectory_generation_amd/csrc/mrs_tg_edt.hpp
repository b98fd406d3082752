// mrs_tg_edt.hpp -- the voxel grid of (signed) distances mrs_tg_plan_field_clearance reads, built from an OCCUPANCY grid by an exact
// Euclidean distance transform (mrs_tg_field_from_occupancy; edt_x_kernel, edt_y_kernel, edt_z_kernel in mrs_tg_edt.hip); DESIGN.md
// section 11l.  Mapping stacks publish occupancy, not distances; mrs_tg_field.hpp's recipe from a list of obstacles costs nodes
// times obstacles.  This costs voxels times a scan that ends early.
//
// occupancy [n_fields][nz][ny][nx] uint8, x fastest, the layout and the mrs_tg_field_geometry of mrs_tg_field.hpp: node-centred,
// grids of one geometry stacked.  A voxel is OCCUPIED when its byte is non-zero ("unknown" is the caller's business).  fields
// [n_fields][nz][ny][nx] doubles is what mrs_tg_plan_field_clearance takes.
//
// The definition, which names no algorithm.  Weights, computed once on the host (weights()):
//   wx = hx hx    wy = hy hy    wz = (z_scale hz) (z_scale hz)
// The squared distance between two nodes of the same grid with integer offsets di, dj, dk:
//   q = (wx (double)(di di) + wy (double)(dj dj)) + wz (double)(dk dk)
// the integer squares exact, the three products and the two sums rounded in this order, nothing fused.  D_occ(v) is the minimum
// of q over the occupied nodes of v's own grid (+inf where there is none), D_free(v) the same over the free nodes; grids never
// see each other.  The value at a node, with rt(D) = min(sqrt(D), max_distance) and sqrt correctly rounded:
//   unsigned (flags = 0):            free  rt(D_occ)    occupied  0.0
//   signed (MRS_TG_FIELD_SIGNED):    free  rt(D_occ)    occupied  -rt(D_free)
// max_distance is positive and may be +inf; with +inf an all-free or all-occupied grid holds +-inf voxels, lerp(inf, inf, t) is
// NaN in mrs_tg_plan_field_clearance, and a caller who looks such a field up passes a finite cap.
//
// Separable in bits.  fl(a + c) is monotone in a, so the minimum over i' of fl(fl(A(i') + b) + c) is fl(fl(min A + b) + c):
//   D1(i, j, k) = min over i' occupied in line (j, k) of wx (i - i')^2          (x pass: no sum, the nearest occupied node wins)
//   D2(i, j, k) = min over j' of D1(i, j', k) + wy (j - j')^2                   (y pass)
//   D3(i, j, k) = min over k' of D2(i, j, k') + wz (k - k')^2                   (z pass)
// and D3 is the brute-force minimum of q, bit for bit (tests/test_edt_host.py holds the harness to tests/edt_util.py's brute
// force, which is not separable).
//
// One array for both transforms.  In every pass a node is its own candidate at offset 0, so the partial D_free of a FREE node is
// exactly 0 (wx 0 = 0 in the x pass, 0 + w 0 = 0 afterwards), and so is the partial D_occ of an occupied node.  The value at a
// node needs D_occ where the node is free and D_free where it is occupied, and a scan needs, of every node p it looks at,
// D_occ(p) = occupied(p) ? 0 : S(p) or D_free(p) = occupied(p) ? S(p) : 0, with S(p) the partial distance of p to the OTHER class.
// So the passes keep S alone, in the output array, with the class in the sign bit (packed(): -S at an occupied node, -0.0
// included), and seen_by() gives a scan the D it asks for -- the same doubles, 0 + t = t exactly, as two arrays would hold.  An
// unsigned field never scans from an occupied node.
//
// The y and z passes scan outward from the node (scan_line): best = D(j); for d = 1, 2, ... with t = w (double)(d d): stop when
// t >= best, else best = min(best, D(j - d) + t, D(j + d) + t).  Exact by construction: D >= 0, so every candidate at offset d or
// beyond is fl(D + t') >= t' >= t >= best and none is strictly smaller (w (double)(d d) is monotone in d).  It ends early
// wherever something is near.
//
// The one extra early exit, on max_distance (saturation()).  Let T = nextafter(fl(max_distance max_distance), +inf): T >=
// max_distance^2 as real numbers, so for a double x >= T the correctly rounded sqrt(x) >= max_distance (rounding is monotone
// and max_distance is a double) and rt(x) = max_distance.  scan_line also stops when t >= T.  Claim: a pass whose input D'
// satisfies, node by node, "D' == D where D < T, D' >= T where D >= T" (D the exact-scan value) returns an output with the same
// property.  Proof: D' >= min(D, T) everywhere and fl(. + t) is monotone, so every candidate the shortened scan looks at is >=
// min(true candidate, T), and the candidates it skips have t >= T, hence true value >= T as well.  If the true minimum m < T, it
// is attained at an offset with t <= m < T from an input D < T, which is D' exactly: the shortened scan sees that very candidate,
// and nothing it sees is smaller than min(m, T) = m.  If m >= T, everything it sees is >= T.  The x pass is exact (D' = D), so
// by induction D3' == D3 where D3 < T and D3' >= T otherwise -- and there rt gives max_distance for both.  With max_distance =
// +inf (or so large that its square overflows) T = +inf and the exit never fires.  The scan is then bounded by max_distance / h
// steps per node, which is what bounds the cost on a sparse map.
//
// Plain double, __host__ __device__, on mrs_tg_hd.hpp alone: tests/host/edt_harness.cpp runs these per-line routines under g++.
// A staged line limits a dim: kMaxDim per axis (the ABI refuses larger dims before any launch).
//
// Out of scope.  The INDEX of the nearest occupied voxel: a tie rule on the rounded total is not separable (two different
// partial sums can round to the same total).  float32 fields.  Sub-voxel surfaces (half-voxel offsets: the distance is between
// nodes).  A gradient of anything: occupancy is discrete.  (A map that changes inside a box: mrs_tg_edt_region.hpp brings the
// field up to date on these routines.)
#pragma once

#include "mrs_tg_hd.hpp"

#ifndef MRS_TG_EDT_TILE_BYTES
#define MRS_TG_EDT_TILE_BYTES 65536  // (an experiment build may say 32768 or 131072: scripts/edt_cost.py)
#endif

namespace mrs_tg {
namespace edtq {

constexpr int kMaxDim = 1024;                  // the largest dim per axis: a staged line of kMaxDim doubles, kTileMin columns wide
constexpr int kChunk = 64;                     // the x pass looks at a line in chunks of one ballot
constexpr int kMaxChunks = kMaxDim / kChunk;
constexpr int kTileBytes = MRS_TG_EDT_TILE_BYTES;  // the LDS a staged tile of lines may take (64 KB: two workgroups share a compute unit)
constexpr int kTileMax = 64;                   // columns (along x) of a staged tile, a power of two: at most a wavefront's lanes,
constexpr int kTileMin = kTileBytes >= 65536 ? 8 : kTileBytes / (kMaxDim * 8);  // at least what a line of kMaxDim leaves room for
constexpr int kSigned = 1;                     // MRS_TG_FIELD_SIGNED
static_assert(kMaxDim % kChunk == 0 && kTileMin >= 1 && (kTileMin & (kTileMin - 1)) == 0 &&
                  (size_t)kMaxDim * kTileMin * sizeof(double) <= (size_t)kTileBytes && kTileBytes <= 160 * 1024,
              "a line of kMaxDim fits a tile, a tile fits a workgroup's LDS");

MRS_TG_HD inline double infinity() {
  MRS_TG_NO_CONTRACT
  return HUGE_VAL;
}

struct Weights {
  double w[3];  // wx, wy, wz
};
// wx = hx hx, wy = hy hy, wz = (z_scale hz) (z_scale hz): on the host, once
inline Weights weights(const double (&h)[3], double z_scale) {
  MRS_TG_NO_CONTRACT
  Weights W;
  W.w[0] = h[0] * h[0];
  W.w[1] = h[1] * h[1];
  const double hz = z_scale * h[2];
  W.w[2] = hz * hz;
  return W;
}
// T of the header comment: on the host, once.  max_distance > 0 (the ABI's check); +inf gives +inf
inline double saturation(double max_distance) {
  MRS_TG_NO_CONTRACT
  const double c2 = max_distance * max_distance;
  return std::nextafter(c2, infinity());
}

// ---- the x pass: the nearest set bit of a line held as ballots of 64 nodes --------------------------------------------------------

// the nodes of chunk c that exist in a line of nx
MRS_TG_HD inline uint64_t chunk_valid(int nx, int c) {
  MRS_TG_NO_CONTRACT
  const int left = nx - c * kChunk;
  return left >= kChunk ? ~0ull : ((1ull << left) - 1ull);
}
MRS_TG_HD inline int last_set(uint64_t m) {  // (m != 0)
  MRS_TG_NO_CONTRACT
  return 63 - __builtin_clzll(m);
}
MRS_TG_HD inline int first_set(uint64_t m) {  // (m != 0)
  MRS_TG_NO_CONTRACT
  return __builtin_ctzll(m);
}
// the last set node of the chunks in front of c and the first of those behind it, as indices in the line; -1 for none
MRS_TG_HD inline int chunk_prev(const uint64_t* masks, int c) {
  MRS_TG_NO_CONTRACT
  for (int b = c - 1; b >= 0; --b)
    if (masks[b]) return b * kChunk + last_set(masks[b]);
  return -1;
}
MRS_TG_HD inline int chunk_next(const uint64_t* masks, int n_chunks, int c) {
  MRS_TG_NO_CONTRACT
  for (int b = c + 1; b < n_chunks; ++b)
    if (masks[b]) return b * kChunk + first_set(masks[b]);
  return -1;
}
// |i - i'| to the nearest set node i' of the line for node i = c kChunk + lane, -1 where the line has none: the chunk's own
// mask at and below / at and above the lane first, then what the other chunks carry in (prev, next)
MRS_TG_HD inline int x_offset(uint64_t mask, int c, int lane, int prev, int next) {
  MRS_TG_NO_CONTRACT
  const uint64_t below = mask & (~0ull >> (63 - lane)), above = mask & (~0ull << lane);
  const int i = c * kChunk + lane;
  const int l = below ? c * kChunk + last_set(below) : prev;
  const int r = above ? c * kChunk + first_set(above) : next;
  int d = -1;
  if (l >= 0) d = i - l;
  if (r >= 0 && (d < 0 || r - i < d)) d = r - i;
  return d;
}
// D1 from that offset
MRS_TG_HD inline double x_value(int d, double wx) {
  MRS_TG_NO_CONTRACT
  return d < 0 ? infinity() : wx * (double)(d * d);
}

// ---- the y and z passes: the outward scan of one node of one staged line -------------------------------------------------------------

// min over p in [0, n) of at(p) + w (double)((j - p)(j - p)), with the two early exits of the header comment.  at(p) >= 0 or +inf.
template <class At>
MRS_TG_HD inline double scan_line(At&& at, int n, int j, double w, double limit) {
  MRS_TG_NO_CONTRACT
  double best = at(j);
  const int reach = j > n - 1 - j ? j : n - 1 - j;
  for (int d = 1; d <= reach; ++d) {
    const double t = w * (double)(d * d);
    if (t >= best || t >= limit) break;
    if (j - d >= 0) {
      const double c = at(j - d) + t;
      if (c < best) best = c;
    }
    if (j + d < n) {
      const double c = at(j + d) + t;
      if (c < best) best = c;
    }
  }
  return best;
}

// ---- both transforms in one array: S, the partial distance to the other class, with the node's class in the sign bit -----------------

MRS_TG_HD inline double packed(double s, bool occupied) {
  MRS_TG_NO_CONTRACT
  return occupied ? -s : s;
}
MRS_TG_HD inline bool packed_occupied(double v) {
  MRS_TG_NO_CONTRACT
  return __builtin_signbit(v) != 0;
}
// what a scan from a node of the class `occupied` sees of a node that holds v: its partial distance where it is of the same
// class, a source at 0 where it is of the other
MRS_TG_HD inline double seen_by(double v, bool occupied) {
  MRS_TG_NO_CONTRACT
  return packed_occupied(v) == occupied ? fabs(v) : 0.0;
}

// ---- the value at a node -----------------------------------------------------------------------------------------------------------

// rt(D) = min(sqrt(D), max_distance)
MRS_TG_HD inline double capped_root(double D, double max_distance) {
  MRS_TG_NO_CONTRACT
  const double r = sqrt(D);
  return r < max_distance ? r : max_distance;
}
// a free node from D_occ; an occupied node from D_free (signed) or 0.0
MRS_TG_HD inline double free_value(double d_occ, double max_distance) {
  MRS_TG_NO_CONTRACT
  return capped_root(d_occ, max_distance);
}
MRS_TG_HD inline double occupied_value(double d_free, double max_distance) {
  MRS_TG_NO_CONTRACT
  return -capped_root(d_free, max_distance);
}

// ---- the staged tile ----------------------------------------------------------------------------------------------------------------

// columns of a tile of lines of n nodes in a grid of nx columns: the widest power of two in [kTileMin, kTileMax] that fits
// kTileBytes, not wider than the first power of two that covers nx
MRS_TG_HD inline int tile_width(int n, int nx) {
  MRS_TG_NO_CONTRACT
  int tx = kTileMax;
  while (tx > kTileMin && (size_t)n * (size_t)tx * sizeof(double) > (size_t)kTileBytes) tx >>= 1;
  while (tx > 1 && (tx >> 1) >= nx) tx >>= 1;
  return tx;
}

}  // namespace edtq
}  // namespace mrs_tg

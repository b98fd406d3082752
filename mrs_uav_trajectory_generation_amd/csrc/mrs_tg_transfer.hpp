// mrs_tg_transfer.hpp -- the transfer plan of the one-call host interface (mrs_tg_solve_batch / solve_batch_samples_only in
// mrs_tg_abi.hip): which arrays a call has, how each one travels, where each one lies in the context's arenas, what the
// caller's masks say about the batch, whether the caller's statement about its positions holds, and the hints a solve hands
// its launchers (RouteHints).  Plain C++17 arithmetic
// without a HIP type or call: mrs_tg_abi.hip enqueues what this header decides, and tests/host/transfer_harness.cpp runs the
// same functions under g++ and the sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/mrs_tg.h"

namespace mrs_tg {

// every slot of an arena starts on a 256-byte boundary
constexpr size_t align_slot(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// Up to kCopyMax flat copies in ONE launch (copy_many_kernel takes the list by value): how mrs_tg_solve_batch moves arrays
// between pinned host memory (which the GPU addresses directly) and the device -- a kernel launch costs the host ~3 us, a
// hipMemcpyAsync 10-25 us.
constexpr int kCopyMax = 8;
struct CopyList {
  const void* src[kCopyMax];
  void* dst[kCopyMax];
  unsigned long long bytes[kCopyMax];
  int n = 0;
  // false: the list is full and the copy was NOT taken (an empty copy is none: true)
  bool add(const void* s, void* d, size_t b) {
    if (b == 0 || s == nullptr || d == nullptr) return true;
    if (n >= kCopyMax) return false;
    src[n] = s;
    dst[n] = d;
    bytes[n] = b;
    ++n;
    return true;
  }
};

// ---- the arrays of a call.  Every one gets its place in ONE device block kept by the context (no allocation per call once a
// batch shape has been seen).  How an array travels depends on where the caller keeps it:
//   * pinned host memory (mrs_tg_host_alloc / mrs_tg_host_register, or any hipHostMalloc'ed block), which the GPU
//     addresses directly: all pinned inputs are gathered by ONE copy kernel, all pinned outputs scattered by one (a
//     kernel launch costs the host ~3 us, a hipMemcpyAsync 10-25 us, and seven of those were half of a 1024-path call).
//     Fixed-times mode with every array pinned needs no copy at all: the solve kernel reads the caller's inputs once and
//     writes the caller's outputs once, over PCIe, while it computes;
//   * pageable memory, small (<= stage_max bytes): packed into the context's pinned staging block, which travels with the
//     pinned arrays in the same copy kernel -- one transfer each way, no synchronisation in between;
//   * pageable memory, large: hipMemcpyAsync on the caller's buffer (the runtime pins the pages in place; staging 3 MB
//     of coefficients through another host copy costs more than that).
// Waypoints travel only when something reads them: the time estimate, or kernels told that the positions are the waypoints
// (MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS).
enum ArrayId { A_WP, A_MASK, A_VALS, A_LIM, A_T, A_C, A_ST, A_COST, A_NS, A_SMP, A_COUNT };
constexpr ArrayId kInputArrays[] = {A_WP, A_MASK, A_VALS, A_LIM};       // uploaded; A_T (seg_times) travels both ways
constexpr ArrayId kOutputArrays[] = {A_C, A_ST, A_COST, A_NS, A_SMP};  // downloaded, and A_T
constexpr ArrayId kUploadOrder[] = {A_WP, A_MASK, A_VALS, A_LIM, A_T};
constexpr ArrayId kDownloadOrder[] = {A_T, A_C, A_ST, A_COST, A_NS, A_SMP};
struct TransferArray {
  const void* src;  // host source (inputs)
  void* dst;        // host destination (outputs)
  size_t bytes;
  void* pinned;     // device-side address of the caller's array when it lives in pinned memory
  bool staged;      // pageable and small: packed through the context's pinned host arena
  size_t off;       // offset in the device arena
  bool present() const { return (src || dst) && bytes; }
};
// The longest copy lists a call builds: one entry per pinned array of the direction plus one for the staged span (pinned
// samples travel by copy_samples_kernel: only the rows a path produced).
constexpr int kUploadCopiesMax = (int)(sizeof(kUploadOrder) / sizeof(kUploadOrder[0])) + 1;
constexpr int kDownloadCopiesMax = (int)(sizeof(kDownloadOrder) / sizeof(kDownloadOrder[0])) - 1 + 1;
static_assert(kUploadCopiesMax <= kCopyMax && kDownloadCopiesMax <= kCopyMax, "a copy list of the one-call interface outgrows CopyList");

// pinned_address(host pointer, bytes) -> the device-side address of a range the GPU addresses as a whole, or null.  An
// absent array and an array of 0 bytes are neither pinned nor staged.
template <class PinnedAddress>
TransferArray classify(const void* src, void* dst, size_t bytes, size_t stage_max, PinnedAddress&& pinned_address) {
  const void* host = src ? src : dst;
  TransferArray a{src, dst, bytes, nullptr, false, 0};
  if (host != nullptr && bytes > 0) {
    a.pinned = pinned_address(host, bytes);
    a.staged = a.pinned == nullptr && bytes <= stage_max;
  }
  return a;
}

// device layout: unstaged inputs | staged inputs | seg_times (in and out) | staged outputs | unstaged outputs: the staged
// arrays of each direction are one contiguous span, and the host arena mirrors [staged inputs | seg_times | staged outputs]
struct TransferLayout {
  size_t span_begin, in_span_end;   // what one copy carries up: the staged inputs (and a staged seg_times)
  size_t out_span_begin, span_end;  // what one copy carries down: (a staged seg_times and) the staged outputs
  size_t device_bytes, host_bytes;
  size_t host_offset(const TransferArray& a) const { return a.off - span_begin; }  // of a staged array, in the host arena
};
inline TransferLayout lay_out(TransferArray (&arr)[A_COUNT]) {
  TransferLayout L{};
  size_t off = 0;
  auto place = [&off](TransferArray& a, size_t bytes) { a.off = off, off += align_slot(bytes); };
  for (ArrayId id : kInputArrays)
    if (!arr[id].staged) place(arr[id], arr[id].bytes);
  L.span_begin = off;
  for (ArrayId id : kInputArrays)
    if (arr[id].staged) place(arr[id], arr[id].bytes);
  const size_t t_off = off;
  place(arr[A_T], arr[A_T].bytes);
  L.in_span_end = arr[A_T].staged ? off : t_off;
  L.out_span_begin = arr[A_T].staged ? t_off : off;
  for (ArrayId id : kOutputArrays)
    if (arr[id].staged) place(arr[id], arr[id].bytes);
  L.span_end = off;
  for (ArrayId id : kOutputArrays)  // (the kernels want a cost buffer even when the caller does not)
    if (!arr[id].staged) place(arr[id], arr[id].bytes ? arr[id].bytes : 8);
  L.device_bytes = off ? off : 256;
  L.host_bytes = L.span_end - L.span_begin;
  return L;
}

// the arrays' half of the zero-copy decision: every array the caller passed is pinned (the fixed-times solve never reads
// the limits: a pageable limits array does not decide this)
inline bool every_array_pinned(const TransferArray (&arr)[A_COUNT]) {
  for (int id = 0; id < A_COUNT; ++id)
    if (id != A_LIM && arr[id].present() && !arr[id].pinned) return false;
  return true;
}

// What the caller's masks and values, which are in host memory here, say about the batch.  Each scan runs only when wanted
// and stops at its first hit.
struct ConstraintScan {
  bool general_patterns;   // a vertex without a position constraint: the general solver
  bool constrained_slots;  // min-snap: an INTERIOR vertex with a constrained derivative slot (a stop_at waypoint)
  bool moving_starts;      // a path that starts from a moving state: non-zero constrained derivatives at its first vertex
};
inline ConstraintScan scan_constraints(int32_t n_paths, const int32_t* so, const uint8_t* mask, const double* vals, int derivative,
                                       bool want_general, bool want_slots, bool want_moving) {
  // (`if (hit) { flag = true; break; }` on local flags on purpose: with the flags in the loop conditions the two scans of a
  // 1024 x 10 batch cost every call one to two microseconds more)
  bool general = false, slots = false, moving = false;
  const size_t nV = (size_t)so[n_paths] + (size_t)n_paths;
  if (want_general)
    for (size_t v = 0; v < nV; ++v)
      if (mask[v * 5] == 0) {
        general = true;
        break;
      }
  if (want_slots && derivative == 4)
    for (int32_t p = 0; p < n_paths && !slots; ++p)
      for (size_t v = (size_t)so[p] + p + 1; v < (size_t)so[p + 1] + p; ++v)
        if (mask[v * 5 + 1] | mask[v * 5 + 2] | mask[v * 5 + 3] | mask[v * 5 + 4]) {
          slots = true;
          break;
        }
  if (want_moving)
    for (int32_t p = 0; p < n_paths && !moving; ++p) {
      const size_t v = (size_t)so[p] + p;
      for (int k = 1; k < 5 && !moving; ++k)
        if (mask[v * 5 + k])
          for (int q = 0; q < 4; ++q) moving = moving || vals[(v * 5 + k) * 4 + q] != 0.0;
    }
  return ConstraintScan{general, slots, moving};
}

// the batches whose outer-loop launch shape depends on a moving start (launch_nonlinear: small batches of 13-15 segments), the
// same condition on both policy routes and in mrs_tg_solve_batch
inline bool wants_moving_starts(int time_alloc_method, size_t n_paths, int max_segments) {
  return time_alloc_method == MRS_TG_TIME_ALLOC_MELLINGER && n_paths <= 1536 && max_segments >= 13 && max_segments <= 15;
}
// shared_device: other batches are in flight on the device, so launch shapes that leave wavefront slots free are preferred over
// the lowest latency of this launch alone (launch_solve_rows).  constrained_slots: the batch may hold vertices with constrained
// derivative slots beside its paths' ends; min-snap launches then use the instantiations that take such vertices
// (launch_solve_quad, launch_solve_quad_group, launch_nonlinear).  moving_starts: some paths start from a moving state (non-zero
// constrained derivatives at their first vertex); launch_nonlinear's choice between the plan's dimension split and lane groups.
struct RouteHints {            // what a call tells the routers beside its batch and options; never a kernel argument
  bool shared_device = false;      // MRS_TG_FLAG_SHARED_DEVICE
  bool constrained_slots = false;  // MRS_TG_FLAG_CONSTRAINED_SLOTS
  bool moving_starts = false;      // the caller saw a moving start AND the shape is one whose route depends on it
};
// the hints of one solve: its option flags, and what its caller saw of its paths' first vertices (a device-resident caller has
// no flag for a moving start and says false)
inline RouteHints route_hints(int flags, bool moving_start_seen, int time_alloc_method, size_t n_paths, int max_segments) {
  RouteHints h;
  h.shared_device = (flags & MRS_TG_FLAG_SHARED_DEVICE) != 0;
  h.constrained_slots = (flags & MRS_TG_FLAG_CONSTRAINED_SLOTS) != 0;
  h.moving_starts = moving_start_seen && wants_moving_starts(time_alloc_method, n_paths, max_segments);
  return h;
}

// MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS on host arrays: the number of vertices whose position is unconstrained or whose
// constrained position differs from the waypoint -- position_mismatch_kernel's criterion (mrs_tg_kernels.hip), bit for bit
// as there: a NaN equals the NaN of the same bits and nothing else, -0.0 differs from 0.0.  O(V), no early exit: the count is
// what the caller is told.
inline long long count_position_mismatches_host(int32_t n_paths, const int32_t* so, const double* wp, const uint8_t* mask,
                                                const double* vals) {
  const size_t nV = n_paths > 0 ? (size_t)so[n_paths] + (size_t)n_paths : 0;
  long long bad = 0;
  for (size_t v = 0; v < nV; ++v)
    bad += mask[v * 5] == 0 || std::memcmp(wp + v * 4, vals + v * 20, 4 * sizeof(double)) != 0;
  return bad;
}

}  // namespace mrs_tg

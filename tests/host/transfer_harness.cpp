// transfer_harness.cpp -- the transfer plan of the one-call host interface (csrc/mrs_tg_transfer.hpp: the array table,
// classify, lay_out, every_array_pinned, scan_constraints, count_position_mismatches_host, CopyList::add, route_hints) and the device arena
// of a policy round (csrc/mrs_tg_policy_host.hpp: policy_round_arena) compiled with plain g++ for the CPU.  "Pinned" is whatever
// the harness says it is: classify takes the question as a callable.  tests/test_transfer_host.py drives it and restates what
// it prints.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/transfer_harness.cpp -o transfer_harness && ./transfer_harness < in
//
// Input (whitespace separated), any number of commands until end of input; one output line per command:
//   enumerate n_paths n_segments sample_capacity
//       every array absent / pinned / staged / large pageable (seg_times never absent), every combination
//       -> number of states, then the violations of each invariant (the list in check_state below)
//   layout stage_max, then per array (table order) state bytes    state: 0 absent, 1 pinned, 2 pageable
//       -> per array staged off host_offset (host_offset -1 unless staged); span_begin in_span_end out_span_begin span_end
//          device_bytes host_bytes every_array_pinned
//   scan n_paths derivative want_general want_slots want_moving, seg_offsets [n_paths + 1], mask [nV][5], values [nV][5][4]
//       -> general_patterns constrained_slots moving_starts
//   mismatch n_paths (0 allowed), seg_offsets [n_paths + 1], waypoints [nV][4], mask [nV][5], values [nV][5][4]
//       -> count_position_mismatches_host: vertices whose position bit is unset or whose constrained position is not, bit for
//          bit, the waypoint ("nan" and "-nan" read as NaNs of either sign bit)
//   arena n_paths n_segments capacity
//       -> the fields of policy_round_arena in order, then in_bytes, samples and total_bytes of policy_round_layout
//   copylist
//       -> kCopyMax, n after kCopyMax + 1 adds, how many adds were refused
//   hints flags moving_start_seen time_alloc_method n_paths max_segments
//       -> route_hints: shared_device constrained_slots moving_starts, then wants_moving_starts of the last three arguments
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_policy_host.hpp"
#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_transfer.hpp"

using namespace mrs_tg;

namespace {

char g_host[A_COUNT];  // a host "array" per id: only its address is looked at
bool g_pinned[A_COUNT];

void* pinned_address(const void* ptr, size_t) {
  const size_t id = (size_t)(static_cast<const char*>(ptr) - g_host);
  return g_pinned[id] ? const_cast<void*>(ptr) : nullptr;
}
bool is_output(int id) { return id >= A_C; }
TransferArray make(int id, bool absent, size_t bytes, size_t stage_max) {
  void* host = absent ? nullptr : &g_host[id];
  return classify(is_output(id) ? nullptr : host, id == A_T || is_output(id) ? host : nullptr, bytes, stage_max, pinned_address);
}

constexpr int kChecks = 9;
// the arrays of `ids` that are staged tile [begin, end) in offset order, with alignment padding only
bool tiles(const TransferArray (&arr)[A_COUNT], const std::vector<int>& ids, size_t begin, size_t end) {
  std::vector<const TransferArray*> in;
  for (int id : ids)
    if (arr[id].staged) in.push_back(&arr[id]);
  for (size_t i = 0; i < in.size(); ++i)
    for (size_t j = i + 1; j < in.size(); ++j)
      if (in[j]->off < in[i]->off) std::swap(in[i], in[j]);
  size_t cursor = begin;
  for (const TransferArray* a : in) {
    if (a->off != cursor) return false;
    cursor += align_slot(a->bytes);
  }
  return cursor == end;
}
void check_state(const TransferArray (&arr)[A_COUNT], const TransferLayout& L, long long (&bad)[kChecks]) {
  for (int i = 0; i < A_COUNT; ++i) {
    const TransferArray& a = arr[i];
    bad[0] += a.off % 256 != 0;                                        // 0: every offset is a multiple of 256
    if (a.bytes) {                                                     // 1: slots disjoint and inside the device block
      bad[1] += a.off + a.bytes > L.device_bytes;
      for (int j = i + 1; j < A_COUNT; ++j)
        bad[1] += arr[j].bytes && a.off < arr[j].off + arr[j].bytes && arr[j].off < a.off + a.bytes;
    }
    if (!a.staged && !is_output(i) && i != A_T) bad[4] += a.off + a.bytes > L.span_begin;  // 4: unstaged inputs before the spans
    if (!a.staged && is_output(i)) bad[5] += a.off < L.span_end;                           // 5: unstaged outputs behind them
    if (a.staged) bad[6] += L.host_offset(a) + a.bytes > L.host_bytes;                     // 6: the host arena holds the staged
    if (is_output(i) && !a.dst) {                                      // 7: an absent output owns at least 8 bytes
      size_t next = L.device_bytes;
      for (const TransferArray& b : arr)
        if (b.off > a.off && b.off < next) next = b.off;
      bad[7] += next - a.off < (a.bytes > 8 ? a.bytes : 8);
    }
  }
  // 2, 3: the staged arrays of each direction tile their span; an unstaged seg_times lies between the two spans
  bad[2] += !tiles(arr, {A_WP, A_MASK, A_VALS, A_LIM, A_T}, L.span_begin, L.in_span_end);
  bad[3] += !tiles(arr, {A_T, A_C, A_ST, A_COST, A_NS, A_SMP}, L.out_span_begin, L.span_end);
  if (!arr[A_T].staged) {
    bad[2] += arr[A_T].off != L.in_span_end;
    bad[3] += arr[A_T].off + align_slot(arr[A_T].bytes) != L.out_span_begin;
  }
  bad[6] += L.host_bytes != L.span_end - L.span_begin;
  bad[8] += L.device_bytes < 256;                                      // 8: never an empty device block
}

void array_bytes(size_t P, size_t nS, size_t cap, size_t (&bytes)[A_COUNT]) {
  const size_t nV = nS + P;
  const size_t b[A_COUNT] = {nV * 32, nV * 5, nV * 160, P * 72, nS * 8, nS * 320, P * 4, P * 8, P * 4, P * cap * 32};
  std::memcpy(bytes, b, sizeof(b));
}

int enumerate() {
  size_t P, nS, cap, bytes[A_COUNT];
  if (std::scanf("%zu %zu %zu", &P, &nS, &cap) != 3) return 2;
  array_bytes(P, nS, cap, bytes);
  long long states = 0, bad[kChecks] = {};
  int st[A_COUNT] = {};  // 0 absent, 1 pinned, 2 staged, 3 large pageable
  st[A_T] = 1;
  for (;;) {
    TransferArray arr[A_COUNT];
    for (int i = 0; i < A_COUNT; ++i) {
      g_pinned[i] = st[i] == 1;
      // an absent input (and absent samples) has no bytes; an absent output keeps the bytes the batch implies, as in a call
      const size_t b = st[i] == 0 && (!is_output(i) || i == A_SMP) ? 0 : bytes[i];
      // staged: the array just fits under stage_max; large: it is one byte over
      arr[i] = make(i, st[i] == 0, b, st[i] == 3 && b ? b - 1 : b);
      if (b && (arr[i].pinned != nullptr) != (st[i] == 1)) return 3;
      if (b && arr[i].staged != (st[i] == 2)) return 3;
    }
    check_state(arr, lay_out(arr), bad);
    ++states;
    int i = 0;
    for (; i < A_COUNT; ++i) {
      if (++st[i] < 4) break;
      st[i] = i == A_T ? 1 : 0;
    }
    if (i == A_COUNT) break;
  }
  std::printf("%lld", states);
  for (long long b : bad) std::printf(" %lld", b);
  std::printf("\n");
  return 0;
}

int layout() {
  size_t stage_max;
  if (std::scanf("%zu", &stage_max) != 1) return 2;
  TransferArray arr[A_COUNT];
  for (int i = 0; i < A_COUNT; ++i) {
    int state;
    size_t bytes;
    if (std::scanf("%d %zu", &state, &bytes) != 2) return 2;
    g_pinned[i] = state == 1;
    arr[i] = make(i, state == 0, bytes, stage_max);
  }
  const TransferLayout L = lay_out(arr);
  for (const TransferArray& a : arr) std::printf("%d %zu %lld ", (int)a.staged, a.off, a.staged ? (long long)L.host_offset(a) : -1ll);
  std::printf("%zu %zu %zu %zu %zu %zu %d\n", L.span_begin, L.in_span_end, L.out_span_begin, L.span_end, L.device_bytes, L.host_bytes,
              (int)every_array_pinned(arr));
  return 0;
}

int scan() {
  int n_paths, derivative, want[3];
  if (std::scanf("%d %d %d %d %d", &n_paths, &derivative, &want[0], &want[1], &want[2]) != 5 || n_paths < 1) return 2;
  std::vector<int32_t> so((size_t)n_paths + 1);
  for (int32_t& x : so)
    if (std::scanf("%d", &x) != 1) return 2;
  const size_t nV = (size_t)so.back() + (size_t)n_paths;
  std::vector<uint8_t> mask(nV * 5);
  std::vector<double> vals(nV * 20);
  for (uint8_t& m : mask)
    if (std::scanf("%hhu", &m) != 1) return 2;
  for (double& v : vals)
    if (std::scanf("%lf", &v) != 1) return 2;
  const ConstraintScan r = scan_constraints(n_paths, so.data(), mask.data(), vals.data(), derivative, want[0], want[1], want[2]);
  std::printf("%d %d %d\n", (int)r.general_patterns, (int)r.constrained_slots, (int)r.moving_starts);
  return 0;
}

int mismatch() {
  int n_paths;
  if (std::scanf("%d", &n_paths) != 1 || n_paths < 0) return 2;
  std::vector<int32_t> so((size_t)n_paths + 1);
  for (int32_t& x : so)
    if (std::scanf("%d", &x) != 1) return 2;
  const size_t nV = n_paths ? (size_t)so.back() + (size_t)n_paths : 0;
  // (exactly sized: a read beyond a batch's last vertex is the sanitizer build's to find)
  std::vector<double> wp(nV * 4), vals(nV * 20);
  std::vector<uint8_t> mask(nV * 5);
  for (double& w : wp)
    if (std::scanf("%lf", &w) != 1) return 2;
  for (uint8_t& m : mask)
    if (std::scanf("%hhu", &m) != 1) return 2;
  for (double& v : vals)
    if (std::scanf("%lf", &v) != 1) return 2;
  std::printf("%lld\n", count_position_mismatches_host(n_paths, so.data(), wp.data(), mask.data(), vals.data()));
  return 0;
}

int arena() {
  size_t A, nS;
  int cap;
  if (std::scanf("%zu %zu %d", &A, &nS, &cap) != 3) return 2;
  const PolicyRoundLayout L = policy_round_layout(A, nS, cap);
  const PolicyRoundArena a = policy_round_arena(L, A, nS, cap);
  std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", a.results, a.mask, a.vals, a.times, a.coeffs, a.cost, a.status,
              a.n_samples, a.rows, a.samples, a.total_bytes, L.in_bytes, L.samples, L.total_bytes);
  return 0;
}

int copylist() {
  static char src[kCopyMax + 1], dst[kCopyMax + 1];
  CopyList cl;
  int refused = 0;
  for (int i = 0; i < kCopyMax + 1; ++i) refused += !cl.add(&src[i], &dst[i], 1);
  for (int i = 0; i < cl.n; ++i)
    if (cl.src[i] != &src[i] || cl.dst[i] != &dst[i] || cl.bytes[i] != 1) return 3;
  std::printf("%d %d %d\n", kCopyMax, cl.n, refused);
  return 0;
}

int hints() {
  int flags, seen, method, max_segments;
  size_t n_paths;
  if (std::scanf("%d %d %d %zu %d", &flags, &seen, &method, &n_paths, &max_segments) != 5) return 2;
  const RouteHints h = route_hints(flags, seen != 0, method, n_paths, max_segments);
  std::printf("%d %d %d %d\n", (int)h.shared_device, (int)h.constrained_slots, (int)h.moving_starts,
              (int)wants_moving_starts(method, n_paths, max_segments));
  return 0;
}

}  // namespace

int main() {
  char cmd[32];
  while (std::scanf("%31s", cmd) == 1) {
    const int rc = !std::strcmp(cmd, "enumerate") ? enumerate()
                   : !std::strcmp(cmd, "layout")  ? layout()
                   : !std::strcmp(cmd, "scan")    ? scan()
                   : !std::strcmp(cmd, "mismatch") ? mismatch()
                   : !std::strcmp(cmd, "arena")   ? arena()
                   : !std::strcmp(cmd, "copylist") ? copylist()
                   : !std::strcmp(cmd, "hints")   ? hints()
                                                   : 2;
    if (rc) return rc;
  }
  return 0;
}

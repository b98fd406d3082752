// mrs_tg_knobs.hpp -- every environment knob of the library, declared once: its name, what its values mean, its default and
// WHEN it is read.  Plain C++17 without HIP (mrs_tg_policy_host.hpp, which g++ compiles for the host harness, includes it).
//
// Two classes, and a knob does not move from one to the other:
//   * read once per process (the value is cached at the first call of the accessor): a getenv per launch is a measurable
//     share of a 3 us launch, and the headline workload is launch-bound;
//   * read at every call (marked "every call"): the tests switch these inside one process (monkeypatch.setenv).
// All are tuning / test knobs; none is needed for normal use.
#pragma once

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>

namespace mrs_tg {
namespace knob {

constexpr int kUnset = INT_MIN;  // what an integer knob without a default of its own returns when the variable is not set

inline long long env_ll(const char* name, long long unset) {
  const char* e = std::getenv(name);
  return e ? std::atoll(e) : unset;
}
inline int env_int(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}
// a switch: any integer but 0 is on
inline bool env_flag(const char* name, bool unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) != 0 : unset;
}
// a switch with a rule of the library behind it: -1 not set (the rule decides), 0 forced off, 1 forced on
inline int env_forced(const char* name) {
  const char* e = std::getenv(name);
  return e ? (std::atoi(e) != 0 ? 1 : 0) : -1;
}

// ---- routing of the fixed-times solve ----
// MRS_TG_ROWS_KERNEL=0: the tile and lane kernels instead of the rows kernel (default 1)
inline bool rows_kernel() { static const bool v = env_flag("MRS_TG_ROWS_KERNEL", true); return v; }
// MRS_TG_ROWS_PIPELINE=0: the closing stages of a pipeline as separate launches (default 1: one launch for small batches)
inline bool rows_pipeline() { static const bool v = env_flag("MRS_TG_ROWS_PIPELINE", true); return v; }
// MRS_TG_ROWS_PPW=1|2: paths per wavefront of the rows kernel (1 -> 1, anything else -> 2); 0 = not set, by batch size
inline int rows_ppw() { static const int v = [] { const int n = env_int("MRS_TG_ROWS_PPW", kUnset); return n == kUnset ? 0 : n == 1 ? 1 : 2; }(); return v; }
// MRS_TG_QUAD_MIN_PATHS=n: paths per launch from which the quad kernel takes over (default 6144)
inline long long quad_min_paths() { static const long long v = env_ll("MRS_TG_QUAD_MIN_PATHS", 6144); return v; }
// MRS_TG_QUAD_ENDS=0: the general step for paths whose end vertices leave slots free, as until round 5 (default 1)
inline bool quad_ends() { static const bool v = env_flag("MRS_TG_QUAD_ENDS", true); return v; }
// MRS_TG_DUO=0: never the two-sided kernel, =1: whenever the pattern allows; not set: by wavefronts per SIMD.  Every call.
inline int duo_forced() { return env_forced("MRS_TG_DUO"); }
// MRS_TG_DUO_UNIFORM=0: no wavefront of the two-sided kernel is treated as uniform (default 1: a wavefront whose eight paths are
// present and of one length takes the forward loop without predicate and exchanges its coefficients through LDS before it
// stores them; same bits either way).  A TEST knob, not a tuning one and not an interface: it exists so that
// tests/test_gpu_duo_bits.py can hold the two roads to the same bits.  Every call.
inline bool duo_uniform() { return env_flag("MRS_TG_DUO_UNIFORM", true); }
// MRS_TG_DUO_STORE_THROUGH=0: every coefficient store of the two-sided kernels is an ordinary one (default 1: in the grouped
// dispatch, the stores of a uniform wavefront's exchange road -- 64 consecutive bytes per segment and instruction -- are
// write-through stores, which leave no dirty lines in L2 for the end of the dispatch to write back; same bytes either way).  A
// TEST knob like the one above, not an interface: tests/test_gpu_duo_store_through.py holds the two to the same bits.  Every call.
inline bool duo_store_through() { return env_flag("MRS_TG_DUO_STORE_THROUGH", true); }
// MRS_TG_DUO_LEAN=0: the grouped two-sided dispatch never takes its lean instantiation (default 1: a batch whose paths all have
// one even length of at least 4 segments and fill every wavefront -- uniform_S, n_paths % 8 == 0 -- with both knobs above on runs
// solve_duo_group_kernel<WP, true>, the same arithmetic without the bookkeeping of partly filled or mixed wavefronts; same bits
// either way).  A TEST knob like the two above: tests/test_gpu_duo_lean.py holds the two to the same bits.  Every call.
inline bool duo_lean() { return env_flag("MRS_TG_DUO_LEAN", true); }
// MRS_TG_TRACE_INSTANTIATIONS=1: the kernel trace and mrs_tg_plan_explain spell an instantiation that otherwise goes by its
// family's name -- the lean one above reads solve_duo_group_kernel<true, true> instead of solve_duo_group_kernel<true> (default
// 0: the names are interface and stay).  A TEST knob: it lets a test tell which instantiation ran.  Every call.
inline bool trace_instantiations() { return env_flag("MRS_TG_TRACE_INSTANTIATIONS", false); }
// MRS_TG_TILE_MAX_PATHS=n: largest batch the tile kernel takes (scripts/sweep_tile.sh); not set: `by_shape`.  Every call.
inline long long tile_max_paths(long long by_shape) { return env_ll("MRS_TG_TILE_MAX_PATHS", by_shape); }

// ---- routing of the nonlinear pipeline ----
// MRS_TG_DIM_SPLIT_MAX_PATHS=n: one lane per dimension up to n paths, lane groups beyond; not set (kUnset): the measured
// cross-overs.  Every call.
inline int dim_split_max_paths() { return env_int("MRS_TG_DIM_SPLIT_MAX_PATHS", kUnset); }
// MRS_TG_ENDS_MIN_SEGMENTS=n: shortest path that gets its S + 4 lanes in the free-end bins (default 2, clamped to >= 2)
inline int ends_min_segments() { static const int v = std::max(2, env_int("MRS_TG_ENDS_MIN_SEGMENTS", 2)); return v; }
// MRS_TG_LEAN=0|1: never / always the lean outer-loop kernels; not set: with lane groups (no dimension split).  Every call.
inline int lean_forced() { return env_forced("MRS_TG_LEAN"); }
// MRS_TG_LEAN_SHARED=0: one-sided lean sweeps only, 1: shared half sweeps where a whole batch takes them, 2 (default): also
// wave by wave inside the mixed kernel (ragged batches)
inline int lean_shared() { static const int v = env_int("MRS_TG_LEAN_SHARED", 2); return v; }
// MRS_TG_REGROUP=0: a call never goes back from the plan's dimension split to lane groups (default 1)
inline bool regroup() { static const bool v = env_flag("MRS_TG_REGROUP", true); return v; }
// MRS_TG_LEAN_WIDE=0|1: never / always the wide lane groups; not set: by residency rounds
inline int lean_wide_forced() { static const int v = env_forced("MRS_TG_LEAN_WIDE"); return v; }
// MRS_TG_LEAN_WIDE_ALL=0: only 13-15 and 29-30 segments move to the next group width (default 1: every path in S + 4 lanes)
inline bool lean_wide_all() { static const bool v = env_flag("MRS_TG_LEAN_WIDE_ALL", true); return v; }
// MRS_TG_LEAN_RESIDENT_BLOCKS=n: workgroups of a queued lean launch, 0 = no queue; not set (kUnset): what the device holds
inline int lean_resident_blocks() { static const int v = env_int("MRS_TG_LEAN_RESIDENT_BLOCKS", kUnset); return v; }
// MRS_TG_WAVE_KERNEL=0: never the wavefront-per-path outer-loop kernel (default 1)
inline bool wave_kernel() { static const bool v = env_flag("MRS_TG_WAVE_KERNEL", true); return v; }
// MRS_TG_MAXIMA_BOUNDS=0: every entry of the segment maxima searched (default 1: certified bounds first)
inline bool maxima_bounds() { static const bool v = env_flag("MRS_TG_MAXIMA_BOUNDS", true); return v; }

// ---- the C ABI's transfers and checks ----
// MRS_TG_VERIFY_FLAGS=1: MRS_TG_FLAG_POSITIONS_ARE_WAYPOINTS is checked on every solve, a blocking check (default 0)
inline bool verify_flags() { static const bool v = env_flag("MRS_TG_VERIFY_FLAGS", false); return v; }
// MRS_TG_STAGE_MAX_BYTES=n: largest pageable array packed into the pinned staging block (default 256 KiB)
inline size_t stage_max_bytes() { static const size_t v = (size_t)env_ll("MRS_TG_STAGE_MAX_BYTES", 256 * 1024); return v; }
// MRS_TG_ZERO_COPY=0: pinned arrays are copied like the others (default 1: the kernels address them directly)
inline bool zero_copy() { static const bool v = env_flag("MRS_TG_ZERO_COPY", true); return v; }
// MRS_TG_POOL_POISON set (to anything): every block the pool hands out is filled with 0xFF bytes first
inline bool pool_poison() { static const bool v = std::getenv("MRS_TG_POOL_POISON") != nullptr; return v; }

// ---- the path-policy layer ----
// MRS_TG_POLICY_DEVICE=0: the rounds' batch-sized work stays on the host; n >= 1: on the device from n active requests on
// (default 64)
inline int policy_device() { static const int v = env_int("MRS_TG_POLICY_DEVICE", 64); return v; }
// MRS_TG_POLICY_THREADS=n: host threads of the policy layer, at least 1 (1 switches them off); 0 = not set, by CPU count
inline int policy_threads() { static const int v = [] { const int n = env_int("MRS_TG_POLICY_THREADS", kUnset); return n == kUnset ? 0 : std::max(1, n); }(); return v; }
// MRS_TG_POLICY_GRAIN=k: k items (at least 1) are enough for a thread, whatever the call site asks for; 0 = not set
inline size_t policy_grain() { static const size_t v = [] { const int n = env_int("MRS_TG_POLICY_GRAIN", kUnset); return n == kUnset ? (size_t)0 : (size_t)std::max(1, n); }(); return v; }
// MRS_TG_POLICY_TRACE=1: where a call's time went, on stderr (default 0)
inline bool policy_trace() { static const bool v = env_flag("MRS_TG_POLICY_TRACE", false); return v; }
// MRS_TG_POLICY_PINNED=0: the rounds' host block in ordinary memory (default 1: the context's pinned scratch)
inline bool policy_pinned() { static const bool v = env_flag("MRS_TG_POLICY_PINNED", true); return v; }

}  // namespace knob
}  // namespace mrs_tg

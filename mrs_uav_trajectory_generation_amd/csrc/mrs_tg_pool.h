// mrs_tg_pool.h -- caching device allocator of the library (internal).
//
// The one-call host interface (mrs_tg_solve_batch, mrs_tg_find_trajectory, mrs_tg_optimize_paths) creates a plan and
// a dozen device buffers per call; hipMalloc / hipFree cost ~0.1 ms each and hipFree synchronises the device, which
// made a 25 us solve a 1.6 ms call.  Freed blocks are kept per device and handed out again (smallest cached block that
// fits and is at most 4x the request).  Contract: a block is returned to the pool only after the stream that used it
// has been synchronised, so a cached block has no work in flight and may be reused on any stream.
//
// Every block but the sampling tables (which have their own retire list, mrs_tg_kernels.hip) is held by a DeviceBlock (Block
// of mrs_tg_block.hpp over this pool), and these are the places that meet the contract for it: mrs_tg_plan_destroy synchronises the context's stream and then deletes the plan with its blocks; the
// one-call interface ends every call with a synchronise (SyncOnExit) before a plan or an arena can go; mrs_tg_destroy
// synchronises before it deletes the context with its arenas; a block that grows while its owner lives is given back behind
// the idle step its ensure() is handed (StreamIdle: the synchronise, whose error is reported); a scoped block
// (count_position_mismatches) leaves its scope behind the synchronise that reads its result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mrs_tg_block.hpp"

namespace mrs_tg {

hipError_t pool_alloc_bytes(void** p, size_t bytes);
void pool_free(void* p);
// hipFree every cached block (all devices); live blocks are unaffected.  Called when the last context is destroyed.
void pool_release_cached();

struct PoolAlloc {
  using Error = hipError_t;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return pool_alloc_bytes(p, bytes); }
  static void free(void* p) { pool_free(p); }
  // (the blocks that take this default are sized by their plan's shape alone and never grow, so it never runs for them)
  static hipError_t idle() { return hipDeviceSynchronize(); }
};
template <class T>
using DeviceBlock = Block<T, PoolAlloc>;

// the idle step of a block that one stream uses: the synchronise, and what it said
struct StreamIdle {
  hipStream_t stream;
  hipError_t operator()() const { return hipStreamSynchronize(stream); }
};

// pinned host memory (hipHostMalloc): hipHostFree waits for the device itself
struct PinnedAlloc {
  using Error = hipError_t;
  static constexpr hipError_t ok = hipSuccess;
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
  static hipError_t idle() { return hipSuccess; }
};

}  // namespace mrs_tg

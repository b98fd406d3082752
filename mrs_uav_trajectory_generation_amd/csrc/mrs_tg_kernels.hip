// mrs_tg_kernels.hip -- gfx950 kernels of the batched trajectory optimiser and their launchers.
//
// Data layout in HBM (DESIGN.md "layout"):
//   * ABI-facing arrays are CSR/AoS exactly as include/mrs_tg.h states;
//   * materialised per-segment blocks (H, A^-1) are slot-major SoA: element e = r*10+c of segment j of
//     the path at sorted position q sits at ((j*100 + e) * P + q), so consecutive lanes (consecutive q)
//     touch consecutive doubles for every (j, e): both the assembly kernel's stores and the solve
//     kernel's loads are fully coalesced without any LDS transposition;
//   * the back-substitution workspace uses the same idea: ((v*42 + e) * P + q).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "mrs_tg_device.hpp"
#include "mrs_tg_estimate.hpp"
#include "mrs_tg_sampling.hpp"
#include "mrs_tg_solve.hpp"
#include "mrs_tg_launch.h"
#include "mrs_tg_pool.h"

namespace mrs_tg {

// ---------------------------------------------------------------------------------------------
// K1: Hessian / mapping-block assembly.  HBM-write bound: 8 B read + 1600 B written per segment.
// One thread per (path position, matrix row, segment slot): blockIdx.z is the slot and blockIdx.y the
// row, so there is no index arithmetic beyond one multiply-add, the row's constants are wave-uniform
// (scalar loads) and every store instruction writes 64 consecutive doubles.  The H row is stored before
// the A^-1 row (which needs the division) is computed, so the stores start one dependent load +
// ~20 multiplies after the wave starts.  Launch shapes measured in scripts/k1_variants.hip
// (1024 x 10: 4.8 us against 4.6 us for a pure fill of the same 16.5 MB and 5.2 us for the previous
// two-paths-per-lane, 16-byte-store shape).

// row a of H(T) = T^(1-2d) D_T HBAR_d D_T
__device__ __forceinline__ void hessian_row(double T, int d, int a, double (&hrow)[kN]) {
  const double t2 = T * T, t3 = t2 * T, t4 = t2 * t2;
  const double w[kHalf] = {1.0, T, t2, t3, t4};
  const int pa = a % kHalf;
  const double td = (d == 0) ? 1.0 : (d == 1) ? T : (d == 2) ? t2 : (d == 3) ? t3 : t4;
  const double wa = (pa == 0) ? 1.0 : (pa == 1) ? T : (pa == 2) ? t2 : (pa == 3) ? t3 : t4;
  const double sa = (T / (td * td)) * wa;  // T^(1-2d) * T^pa
#pragma unroll
  for (int c = 0; c < kN; ++c) hrow[c] = c_hbar[d][a][c] * sa * w[c % kHalf];
}

// row a of A^-1(T): ABAR_INV[a][c] * T^(c%5) / T^a
__device__ __forceinline__ void mapping_inverse_row(double T, int a, double (&arow)[kN]) {
  const double t2 = T * T, t3 = t2 * T, t4 = t2 * t2;
  const double w[kHalf] = {1.0, T, t2, t3, t4};
  const double ti = 1.0 / T;
  double tia = 1.0;
  for (int k = 0; k < a; ++k) tia *= ti;
#pragma unroll
  for (int c = 0; c < kN; ++c) arow[c] = c_abar_inv[a][c] * w[c % kHalf] * tia;
}

// The blocks leave as STREAMING stores (round 6): 1 600 bytes per segment that the kernel itself never reads again.  Marked
// non-temporal, a 16.5 MB launch takes 5.3 instead of 5.9 us (0.385 instead of 0.35 of the HBM peak), a 1.05 GB launch 154-157
// instead of 161-165 us (0.84-0.85); the step that solves from the blocks right behind it finds fewer of them in the L2 and is
// 0.5 us slower (12.7-13.5 -> 13.1-14.0 us per 1024 x 10 step).  (Ordinary stores until round 5.)
__device__ __forceinline__ void store_block_rows(double T, int d, int a, size_t base, size_t P, double* __restrict__ Hout,
                                                 double* __restrict__ Aout) {
  double row[kN];
  hessian_row(T, d, a, row);
#pragma unroll
  for (int c = 0; c < kN; ++c) __builtin_nontemporal_store(row[c], &Hout[base + (size_t)c * P]);
  mapping_inverse_row(T, a, row);
#pragma unroll
  for (int c = 0; c < kN; ++c) __builtin_nontemporal_store(row[c], &Aout[base + (size_t)c * P]);
}

// general (ragged) batches: slot j holds the first slot_start[j+1] - slot_start[j] positions of the
// longest-first order; blocks beyond that count exit at once
__global__ __launch_bounds__(256) void assemble_blocks_kernel(BatchView b, int d, const double* __restrict__ seg_times,
                                                              double* __restrict__ Hout, double* __restrict__ Aout) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int j = blockIdx.z;
  if (q >= b.slot_start[j + 1] - b.slot_start[j]) return;
  const int a = blockIdx.y;
  const int p = b.order[q];
  const double T = seg_times[b.seg_offsets[p] + j];
  const size_t P = (size_t)b.n_paths;
  store_block_rows(T, d, a, ((size_t)j * 100 + (size_t)a * kN) * P + (size_t)q, P, Hout, Aout);
}

// uniform batches (every path has S segments, so position q == path q and segment (q, j) sits at q*S + j):
// no indirection loads
// One-dimensional grid of (path chunk, row, slot) workgroups, the chunk slowest, numbered so that each XCD owns a
// contiguous range (xcd_contiguous_index): the XCD that writes the blocks of paths [128 c, 128 c + 128) is then the XCD
// whose tiles of the solve kernel read them (same partition of the paths over the XCDs), and finds them in its own L2.
constexpr int kAssembleChunk = 128;
__global__ __launch_bounds__(kAssembleChunk) void assemble_blocks_uniform_kernel(int n_paths, int S, int d,
                                                                                 const double* __restrict__ seg_times,
                                                                                 double* __restrict__ Hout,
                                                                                 double* __restrict__ Aout) {
  // Which workgroup writes what.  Small launches (the headline's 1024 paths: 8 chunks): workgroups of one chunk of paths are
  // neighbours in the XCD-contiguous numbering, so the XCD that writes the blocks of a chunk is the one whose solve tiles read
  // them.  Large launches: the CHUNK varies fastest -- the workgroups in flight then write neighbouring 1 KB runs of the same few
  // rows instead of runs scattered over the whole gigabyte (twenty arrays 512 KB apart per workgroup): 65536 x 10 on buffers the
  // driver placed badly 0.63-0.66 -> 0.73-0.75 of the HBM peak, on well-placed ones 0.78 -> 0.80 (round 6,
  // profiles/round6_assembly_placement.txt, whose A / B builds ran the first / second order at every size)
  const int n_chunks = (n_paths + kAssembleChunk - 1) / kAssembleChunk;
  const bool chunk_fastest = n_chunks >= 64;
  int chunk, rem;
  if (chunk_fastest) {
    const int logical = (int)blockIdx.x;
    rem = logical / n_chunks;
    chunk = logical - rem * n_chunks;
  } else {
    const int logical = xcd_contiguous_index(blockIdx.x, gridDim.x);
    const int per_chunk = kN * S;
    chunk = logical / per_chunk;
    rem = logical - chunk * per_chunk;
  }
  const int j = rem / kN, a = rem - j * kN;
  const int q = chunk * kAssembleChunk + threadIdx.x;
  if (q >= n_paths) return;
  const double T = seg_times[(size_t)q * S + j];
  const size_t P = (size_t)n_paths;
  store_block_rows(T, d, a, ((size_t)j * 100 + (size_t)a * kN) * P + (size_t)q, P, Hout, Aout);
}

// ---------------------------------------------------------------------------------------------
// K2: linear QP solve (mrs_tg_solve.hpp).  ND = 4: one lane per path; ND = 1: four lanes per path.
// FUSED = false consumes the materialised blocks written by K1, FUSED = true recomputes them from T.

template <int ND, bool FUSED>
__global__ __launch_bounds__(64) void solve_linear_kernel(BatchView b, int d, const uint8_t* __restrict__ mask,
                                                          const double* __restrict__ vals,
                                                          const double* __restrict__ seg_times,
                                                          const double* __restrict__ Hblk, const double* __restrict__ Ablk,
                                                          double* __restrict__ ws, double* __restrict__ coeffs,
                                                          int32_t* __restrict__ status, double* __restrict__ cost,
                                                          const int32_t* __restrict__ status_in) {
  constexpr int LPP = kD / ND;  // lanes per path
  const int tid = blockIdx.x * 64 + threadIdx.x;
  const int lanes_total = b.n_paths * LPP;
  if (tid >= lanes_total) return;
  const int q = tid / LPP;
  const int dim0 = (tid % LPP) * ND;
  const PathRef pr = path_at(b, q);
  BlockSource src{Hblk, Ablk, (size_t)b.n_paths, q};
  bool pos_ok;
  double c = solve_path<ND, FUSED>(mask, vals, pr.v0, pr.S, d, seg_times + pr.s0, dim0, src, ws, (size_t)lanes_total,
                                   (unsigned)tid, coeffs + (size_t)pr.s0 * kD * kN, pos_ok);
  if (LPP == 4) {
    c += __shfl_xor(c, 1, 64);
    c += __shfl_xor(c, 2, 64);
  }
  if (dim0 == 0) {
    if (cost) cost[pr.p] = c;
    if (status) status[pr.p] = merge_status(pos_ok, status_in, pr.p);
  }
}

// ---------------------------------------------------------------------------------------------
// segment-time initialisation: estimateSegmentTimesEuclidean
// (/root/reference/src/eth_trajectory_generation/vertex.cpp:491-565), one thread per segment

__global__ __launch_bounds__(256) void estimate_times_kernel(BatchView b, const double* __restrict__ wp,
                                                             const double* __restrict__ limits,
                                                             double* __restrict__ seg_times) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= b.n_segments) return;
  // path_of_segment(b, idx) of mrs_tg_batch.hpp, written out: through the function the compiler places the loads of b differently
  int p;
  if (b.uniform_S > 0) {
    p = idx / b.uniform_S;
  } else {
    int lo = 0, hi = b.n_paths;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (b.seg_offsets[mid] <= idx) lo = mid;
      else hi = mid;
    }
    p = lo;
  }
  const int v = idx + p;  // vertex index of the segment's start
  seg_times[idx] = estimate_segment_time(wp + (size_t)v * 4, limits + (size_t)p * 9);
}

// ---------------------------------------------------------------------------------------------
// sampler: Trajectory::evaluateRange's accumulate-and-carry walk
// (/root/reference/src/eth_trajectory_generation/trajectory.cpp:93-151), positions + wrapped heading
// (the only fields the nodelet reads, src/mrs_trajectory_generation.cpp:1582-1599).
//
// The reference's sample times are defined by repeated floating-point addition
// (time_in_segment += dt; accumulated += dt, with the remainder carried into the next segment), so the
// sample count and the segment a boundary sample falls into depend on that exact rounding.  One wavefront
// per path walks the trajectory a chunk of up to 64 samples at a time: lane j adds dt to the chunk's start
// values j times -- the same additions in the same order as the reference's running sums, so its
// time_in_segment / accumulated values are bit-identical to those of the reference's j-th next sample -- a ballot
// finds the first lane at which the walk stops (segment end, trajectory end or capacity), the lanes before it
// evaluate the four polynomials of the current segment and store their sample, and the stopping lane's values
// seed the next chunk.  A serial replay on one lane cost ~190 shader cycles per sample (divergent-branch
// control flow around three compares); the chunked walk costs ~20.
// The heading goes through the reference's quaternion round trip, atan2(2wz, 1-2z^2) with
// w = cos(y/2), z = sin(y/2) (eth_mav_msgs/common.h:130-140), which is the wrap of y to (-pi, pi];
// it is computed as y - 2 pi rint(y / 2 pi) (agreement 1e-15; same value at the +-pi seam).
// A trajectory longer than the caller's capacity is reported as capacity + 1 samples ("too long": the
// nodelet rejects such results by its length check, src/mrs_trajectory_generation.cpp:1178-1199); this
// bounds the walk, which matters because a path whose outer loop ended on a rejected trial point
// can come back with segment times of thousands of seconds.

template <int NDER>
__global__ __launch_bounds__(64) void sample_kernel(BatchView b, const double* __restrict__ coeffs,
                                                    const double* __restrict__ seg_times, double dt, int capacity,
                                                    int32_t* __restrict__ n_samples, double* __restrict__ samples,
                                                    const double* __restrict__ acc_table, int acc_n) {
  extern __shared__ double s_T[];  // [max_segments] segment times | [S][4][10] coefficients of this path | sample buffer
  const int lane = threadIdx.x;
  double* s_c = s_T + b.max_segments;
  double* s_t = s_c + (size_t)b.max_segments * kD * kN;                         // [kSampleBuffer] time in segment
  unsigned short* s_seg = reinterpret_cast<unsigned short*>(s_t + kSampleBuffer);  // [kSampleBuffer] segment index
  // (a launch may carry fewer workgroups than paths: a workgroup then walks the paths q, q + gridDim.x, ...)
  for (int q = blockIdx.x; q < b.n_paths; q += gridDim.x) {
    const PathRef pr = path_at(b, q);
    const int S = pr.S;
    MRS_TG_PHASE_MARK(0);
    for (int i = lane; i < S; i += 64) s_T[i] = seg_times[pr.s0 + i];
    if (samples) {  // one coalesced pass instead of a global round trip per segment inside the walk
      const double* __restrict__ cg = coeffs + (size_t)pr.s0 * kD * kN;
      for (int e = lane; e < S * kD * kN; e += 64) s_c[e] = cg[e];
    }
    __syncthreads();
    MRS_TG_PHASE_MARK(1);
    double* out = samples ? samples + (size_t)pr.p * capacity * (NDER + 1) * kD : nullptr;
    const int n = sample_path_walk<NDER>(s_T, s_c, s_t, s_seg, S, dt, capacity, out, acc_table, acc_n);
    MRS_TG_PHASE_MARK(2);
    if (lane == 0 && n_samples) n_samples[pr.p] = n;
    __syncthreads();  // (the next path's staging overwrites what this walk read)
  }
}

// ---------------------------------------------------------------------------------------------
// launchers

hipError_t launch_assemble(const BatchView& b, int d, const double* seg_times, double* H, double* Ainv,
                           hipStream_t stream) {
  if (b.n_segments == 0) return hipSuccess;
  if (b.uniform_S > 0) {
    dim3 grid(cdiv(b.n_paths, kAssembleChunk) * kN * b.uniform_S);
    MRS_TG_LAUNCH_TIMED(assemble_blocks_uniform_kernel, grid, dim3(kAssembleChunk), 0, stream, b.n_paths, b.uniform_S, d,
                        seg_times, H, Ainv);
  } else {
    dim3 grid(cdiv(b.n_paths, 256), kN, b.max_segments);
    MRS_TG_LAUNCH_TIMED(assemble_blocks_kernel, grid, dim3(256), 0, stream, b, d, seg_times, H, Ainv);
  }
  return hipGetLastError();
}

// the dispatcher over the route's family (route_solve, mrs_tg_solve_route.hpp); the lane kernel's launch is its own
hipError_t launch_solve_linear(const BatchView& b, const SolveRoute& route, const SolveOperands& op, hipStream_t stream,
                               const RowsTail& tail) {
  switch (route.family) {
    case SolveFamily::kNone: return route.group == 0 ? hipSuccess : hipErrorInvalidValue;
    case SolveFamily::kDuo:
    case SolveFamily::kQuad: return route.group == 0 ? launch_solve_quad(b, route, op, stream, tail) : hipErrorInvalidValue;
    case SolveFamily::kRows:
    case SolveFamily::kRowsPipeline: return route.group == 0 ? launch_solve_rows(b, route, op, stream, tail) : hipErrorInvalidValue;
    case SolveFamily::kTile: return launch_solve_tile(b, route, op, stream);
    case SolveFamily::kLane: break;
  }
  // (the parentheses are part of the names these launches have always noted)
  const auto linear = route.lanes_per_path == 1 ? MRS_TG_KERNEL((solve_linear_kernel<4, true>))
                      : route.fused             ? MRS_TG_KERNEL((solve_linear_kernel<1, true>))
                                                : MRS_TG_KERNEL((solve_linear_kernel<1, false>));
  MRS_TG_LAUNCH_TIMED(linear, dim3(route.grid_x), dim3(route.threads), 0, stream, b, route.derivative, op.mask, op.vals, op.seg_times,
                      op.H, op.Ainv, op.ws, op.coeffs, op.status, op.cost, op.status_in);
  return hipGetLastError();
}

// blockIdx.y = entry of the list; 16-byte words where both ends are 16-byte aligned (every array of the ABI in practice),
// narrower words otherwise; grid-stride, so that a few hundred workgroups keep enough PCIe reads / writes in flight
__global__ __launch_bounds__(256) void copy_many_kernel(CopyList cl) {
  const int e = blockIdx.y;
  const char* src = static_cast<const char*>(cl.src[e]);
  char* dst = static_cast<char*>(cl.dst[e]);
  const unsigned long long bytes = cl.bytes[e];
  const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long align = (unsigned long long)(uintptr_t)src | (unsigned long long)(uintptr_t)dst;
  unsigned long long done = 0;
  if ((align & 15ull) == 0) {
    const unsigned long long n = bytes >> 4;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (unsigned long long i = tid; i < n; i += stride) d4[i] = s4[i];
    done = n << 4;
  } else if ((align & 7ull) == 0) {
    const unsigned long long n = bytes >> 3;
    const unsigned long long* s8 = reinterpret_cast<const unsigned long long*>(src);
    unsigned long long* d8 = reinterpret_cast<unsigned long long*>(dst);
    for (unsigned long long i = tid; i < n; i += stride) d8[i] = s8[i];
    done = n << 3;
  } else if ((align & 3ull) == 0) {
    const unsigned long long n = bytes >> 2;
    const unsigned* s32 = reinterpret_cast<const unsigned*>(src);
    unsigned* d32 = reinterpret_cast<unsigned*>(dst);
    for (unsigned long long i = tid; i < n; i += stride) d32[i] = s32[i];
    done = n << 2;
  }
  for (unsigned long long i = done + tid; i < bytes; i += stride) dst[i] = src[i];
}

__global__ __launch_bounds__(256) void copy_samples_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                           const int32_t* __restrict__ n_samples, int n_paths, int capacity) {
  for (int p = blockIdx.x; p < n_paths; p += gridDim.x) {
    const int n = min(n_samples[p], capacity);
    const size_t base = (size_t)p * (size_t)capacity * kD;
    const double2* s2 = reinterpret_cast<const double2*>(src + base);  // a row of four doubles = two 16-byte words
    double2* d2 = reinterpret_cast<double2*>(dst + base);
    for (int e = threadIdx.x; e < 2 * n; e += blockDim.x) d2[e] = s2[e];
  }
}

hipError_t launch_copy_samples(const double* src, double* dst, const int32_t* n_samples, int n_paths, int capacity,
                               hipStream_t stream) {
  if (n_paths <= 0 || capacity <= 0) return hipSuccess;
  MRS_TG_LAUNCH(copy_samples_kernel, dim3((unsigned)(n_paths < 2048 ? n_paths : 2048)), dim3(256), 0, stream, src, dst,
                     n_samples, n_paths, capacity);
  return hipGetLastError();
}

hipError_t launch_copy_many(const CopyList& cl, hipStream_t stream) {
  if (cl.n == 0) return hipSuccess;
  unsigned long long most = 0;
  for (int i = 0; i < cl.n; ++i) most = cl.bytes[i] > most ? cl.bytes[i] : most;
  // one 16-byte word per thread up to 512 workgroups, grid-stride beyond
  unsigned blocks = (unsigned)((most / 16 + 255) / 256);
  blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks);
  MRS_TG_LAUNCH(copy_many_kernel, dim3(blocks, (unsigned)cl.n), dim3(256), 0, stream, cl);
  return hipGetLastError();
}

hipError_t launch_estimate_times(const BatchView& b, const double* wp, const double* limits, double* seg_times,
                                 hipStream_t stream, bool timed) {
  if (b.n_segments == 0) return hipSuccess;
  if (timed)
    MRS_TG_LAUNCH_TIMED(estimate_times_kernel, dim3(cdiv(b.n_segments, 256)), dim3(256), 0, stream, b, wp, limits, seg_times);
  else
    MRS_TG_LAUNCH(estimate_times_kernel, dim3(cdiv(b.n_segments, 256)), dim3(256), 0, stream, b, wp, limits,
                     seg_times);
  return hipGetLastError();
}

// The accumulated time of the reference's sampling walk, A[k] = k additions of dt to 0 (mrs_tg_sampling.hpp).  One lane makes
// the additions the reference makes, in its order (IEEE double, round to nearest: v_add_f64) -- a dependent chain of n
// additions, ~20 us for 4096 entries, once per (device, dt).
__global__ void sample_acc_table_kernel(double* __restrict__ table, int n, double dt) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0.0;
  for (int k = 0; k < n; ++k) {
    table[k] = acc;
    acc += dt;
  }
}

// Cache of those tables, per (device, bit pattern of dt).  Everything a call does here is ordered on ITS stream and legal
// under stream capture once the table exists (the first version ran hipMalloc + a synchronous hipMemcpy inside
// the launch path, never evicted, and leaked outgrown tables):
//   * a table is built by a kernel on the calling stream, from a block of the library's pool; an event recorded behind the
//     build is what a launch on ANOTHER stream waits for (hipStreamWaitEvent) until the build has been seen complete once;
//   * at most kAccCacheMax tables are kept; the least recently used one is retired when a new dt arrives, and a table that
//     is outgrown (a larger capacity) is retired too.  A retired table may still be read by a launch in flight on some
//     stream, so it is parked; when kAccRetiredMax tables are parked the device is synchronised ONCE and all of them go back
//     to the pool -- a host that derives a new dt per request pays one device synchronisation per 64 requests and holds at
//     most 96 small tables;
//   * sample_tables_release() (the last context of the process is destroyed) frees everything.
namespace {
struct AccBlock {  // a table's memory: lives until no cache entry names it AND no launch that was handed it is still to be enqueued
  double* d = nullptr;
  int device = 0;
  int pins = 0;  // (under g_acc_mu) callers between sample_acc_table's return and the enqueue of their kernel
};
struct AccEntry {
  AccBlock* blk = nullptr;
  int n = 0;
  hipEvent_t ready = nullptr;  // recorded behind the build
  hipStream_t built_on = nullptr;
  bool ready_seen = false;
  unsigned long long stamp = 0;
};
constexpr size_t kAccCacheMax = 32, kAccRetiredMax = 64;
std::mutex g_acc_mu;
std::map<std::pair<int, unsigned long long>, AccEntry> g_acc_cache;
std::vector<AccBlock*> g_acc_retired;
unsigned long long g_acc_clock = 0;

void acc_retire(AccEntry& en) {
  if (en.ready) (void)hipEventDestroy(en.ready);
  if (en.blk) g_acc_retired.push_back(en.blk);
  en = AccEntry{};
}

// (g_acc_mu held) After the synchronisations no ENQUEUED launch reads a parked table; a table some caller still holds a pin
// on -- handed out, its kernel not enqueued yet -- stays parked for the next drain.  A device synchronisation is illegal while
// the calling stream records a graph: the parked list then simply grows until a call outside a capture drains it.
void acc_drain_retired(hipStream_t stream) {
  if (g_acc_retired.empty()) return;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (stream != nullptr && hipStreamIsCapturing(stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return;
  (void)hipGetLastError();
  int cur = 0;
  (void)hipGetDevice(&cur);
  int last = -1;
  std::vector<AccBlock*> kept;
  for (AccBlock* r : g_acc_retired) {
    if (r->pins > 0) {
      kept.push_back(r);
      continue;
    }
    if (r->device != last) {
      (void)hipSetDevice(r->device);
      (void)hipDeviceSynchronize();
      last = r->device;
    }
    pool_free(r->d);
    delete r;
  }
  g_acc_retired.swap(kept);
  (void)hipSetDevice(cur);
}
}  // namespace

AccPin::~AccPin() {
  if (!block) return;
  std::lock_guard<std::mutex> lock(g_acc_mu);
  --static_cast<AccBlock*>(block)->pins;
}

void sample_tables_release() {
  std::lock_guard<std::mutex> lock(g_acc_mu);
  for (auto& kv : g_acc_cache) acc_retire(kv.second);
  g_acc_cache.clear();
  acc_drain_retired(nullptr);
}

hipError_t sample_acc_table(double dt, int capacity, hipStream_t stream, const double** table_out, int* n_out, AccPin* pin) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  unsigned long long bits;
  static_assert(sizeof(bits) == sizeof(dt), "dt as a key");
  std::memcpy(&bits, &dt, sizeof(bits));
  const int need = (capacity > 0 ? capacity : 0) + 80;
  std::lock_guard<std::mutex> lock(g_acc_mu);
  const auto key = std::make_pair(dev, bits);
  auto it = g_acc_cache.find(key);
  if (it == g_acc_cache.end() || it->second.n < need) {
    if (it == g_acc_cache.end()) {
      if (g_acc_cache.size() >= kAccCacheMax) {  // retire the least recently used table
        auto lru = g_acc_cache.begin();
        for (auto j = g_acc_cache.begin(); j != g_acc_cache.end(); ++j)
          if (j->second.stamp < lru->second.stamp) lru = j;
        acc_retire(lru->second);
        g_acc_cache.erase(lru);
      }
      it = g_acc_cache.emplace(key, AccEntry{}).first;
    } else {
      acc_retire(it->second);  // outgrown
    }
    if (g_acc_retired.size() >= kAccRetiredMax) acc_drain_retired(stream);
    AccEntry& en = it->second;
    int n = 1024 + 80;
    while (n < need) n *= 2;  // (growth by doubling: a caller that raises its capacity step by step rebuilds log2 times)
    en.blk = new (std::nothrow) AccBlock();
    if (!en.blk) {
      g_acc_cache.erase(it);
      return hipErrorOutOfMemory;
    }
    en.blk->device = dev;
    if ((e = pool_alloc_bytes(reinterpret_cast<void**>(&en.blk->d), sizeof(double) * (size_t)n)) != hipSuccess) {
      delete en.blk;
      g_acc_cache.erase(it);
      return e;
    }
    en.n = n;
    MRS_TG_LAUNCH(sample_acc_table_kernel, dim3(1), dim3(64), 0, stream, en.blk->d, n, dt);
    if ((e = hipGetLastError()) == hipSuccess) e = hipEventCreateWithFlags(&en.ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(en.ready, stream);
    if (e != hipSuccess) {
      acc_retire(en);
      g_acc_cache.erase(it);
      return e;
    }
    en.built_on = stream;
  }
  AccEntry& en = it->second;
  en.stamp = ++g_acc_clock;
  if (!en.ready_seen) {
    if (hipEventQuery(en.ready) == hipSuccess) {
      en.ready_seen = true;
    } else if (stream != en.built_on) {  // (the building stream itself is ordered behind the build)
      (void)hipGetLastError();
      if ((e = hipStreamWaitEvent(stream, en.ready, 0)) != hipSuccess) return e;
    }
  }
  *table_out = en.blk->d;
  *n_out = en.n;
  if (pin && !pin->block) {  // the caller's launch is not enqueued yet: the block may be retired meanwhile, not recycled
    pin->block = en.blk;
    ++en.blk->pins;
  }
  return hipSuccess;
}

// One wavefront per path at every size.  (A sampler of 8 or 16 lanes per path, walk and evaluation fused, was built in round 6 and
// measured slower everywhere; it is gone, the record is profiles/round6_sampler_group_ab.txt.)
template <int NDER>
static hipError_t launch_sample_n(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                                  int32_t* n_samples, double* samples, hipStream_t stream) {
  const double* acc_table = nullptr;
  int acc_n = 0;
  AccPin pin;  // (released when this function returns: behind the enqueue of the kernel that reads the table)
  if (!dry_run()) {  // (a dry run builds no table: an entry whose build kernel was not enqueued must not enter the cache)
    hipError_t et = sample_acc_table(dt, capacity, stream, &acc_table, &acc_n, &pin);
    if (et != hipSuccess) return et;
  }
  const size_t lds = sizeof(double) * ((size_t)b.max_segments * (1 + kD * kN) + kSampleBuffer) + sizeof(unsigned short) * kSampleBuffer;
  const auto sampler = MRS_TG_KERNEL(sample_kernel<NDER>);
  if (hipError_t e = prepare_dynamic_lds(sampler, lds); e != hipSuccess) return e;
  // one workgroup per path.  (Fewer, persistent workgroups that walk several paths each -- the kernel's loop allows it --
  // were measured in round 5: 65536 x 10 pipeline 1328 -> 1347 / 1385 / 1384 us with 15360 / 7680 / 3840 workgroups.)
  MRS_TG_LAUNCH(sampler, dim3((unsigned)b.n_paths), dim3(64), lds, stream, b, coeffs, seg_times, dt, capacity,
                     n_samples, samples, acc_table, acc_n);
  return hipGetLastError();
}

hipError_t launch_sample(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                         int32_t* n_samples, double* samples, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  return launch_sample_n<0>(b, coeffs, seg_times, dt, capacity, n_samples, samples, stream);
}

hipError_t launch_sample_states(const BatchView& b, const double* coeffs, const double* seg_times, double dt, int capacity,
                                int32_t* n_samples, double* states, hipStream_t stream) {
  if (b.n_paths == 0) return hipSuccess;
  return launch_sample_n<kSampleStateOrders - 1>(b, coeffs, seg_times, dt, capacity, n_samples, states, stream);
}

__global__ void position_mismatch_kernel(int n_vertices, const double* __restrict__ wp, const uint8_t* __restrict__ mask,
                                         const double* __restrict__ vals, unsigned long long* __restrict__ count) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (v < n_vertices) {
    bad = mask[(size_t)v * kHalf] == 0;
#pragma unroll
    for (int q = 0; q < kD; ++q)  // bitwise: the solve must not depend on which array it read
      bad = bad || __double_as_longlong(wp[(size_t)v * kD + q]) != __double_as_longlong(vals[(size_t)v * kHalf * kD + q]);
  }
  const unsigned long long n = __popcll(__ballot(bad));
  if ((threadIdx.x & 63) == 0 && n != 0) atomicAdd(count, n);
}

hipError_t count_position_mismatches(const BatchView& b, const double* wp, const uint8_t* mask, const double* vals,
                                     hipStream_t stream, long long* count_out) {
  *count_out = 0;
  const int n_vertices = b.n_segments + b.n_paths;
  if (n_vertices == 0) return hipSuccess;
  DeviceBlock<unsigned long long> d_count;  // (leaves the scope behind the synchronise below)
  hipError_t e = d_count.ensure(1);
  if (e != hipSuccess) return e;
  unsigned long long h = 0;
  e = hipMemsetAsync(d_count.get(), 0, sizeof(unsigned long long), stream);
  if (e == hipSuccess) {
    MRS_TG_LAUNCH(position_mismatch_kernel, dim3(cdiv(n_vertices, 256)), dim3(256), 0, stream, n_vertices, wp, mask, vals,
                  d_count.get());
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d_count.get(), sizeof(h), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  *count_out = (long long)h;
  return e;
}

size_t linear_workspace_doubles(const BatchView& b) {
  // worst case: four lanes per path, ws_per_vertex<1>() doubles each
  return (size_t)b.max_segments * ws_per_vertex<1>() * 4 * (size_t)b.n_paths;
}

}  // namespace mrs_tg

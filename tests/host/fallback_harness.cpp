// fallback_harness.cpp -- the fallback sampler, its backward pass and the heading unwrap (csrc/mrs_tg_fallback.hpp: the row rule,
// the rows and the sums fallback_sample_kernel, fallback_sample_vjp_kernel and unwrap_headings_kernel run) compiled with plain
// g++ for the CPU, one path after the other.  tests/test_fallback_host.py checks it against the oracle's mto_fallback_sampling
// and a restatement of the reference's loop; tests/test_gpu_fallback.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/fallback_harness.cpp -o fallback_harness && ./fallback_harness < in
//
// Input (whitespace separated), any number of problems until end of input, S >= 1 segments each:
//   1 S capacity dt stopping_time has_upstream  waypoints [S + 1][4]  stop_at [S + 1]  seg_times [S]  (upstream [capacity][4])
//     -> one line: count (not saturated), n_samples (saturated), seg_first_row [S] (saturated), the min(count, capacity) rows
//        [4] each, and with an upstream dL/dwaypoints [S + 1][4]
//   2 S capacity dt stopping_time relax speed_factor accel_factor  waypoints [S + 1][4]  stop_at [S + 1]  limits [9]
//     -> one line: the whole findTrajectoryFallback: the unwrapped headings [S + 1], the Baca times [S], count, the rows
//   a refused argument (dt, stopping_time, the insert, capacity) -> the line "invalid"
// Doubles are printed with 17 significant digits: the bits survive.
#include <cfloat>
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_fallback.hpp"

namespace fb = mrs_tg::fbq;
namespace bc = mrs_tg::baca;

static bool read(std::vector<double>& v) {
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}

// phase A, then every row below min(count, capacity) found through segment_of_row as a lane of the kernel finds it
static long long sample(const std::vector<double>& w, const std::vector<uint8_t>& stop, const std::vector<double>& t, int S,
                        double dt, int32_t insert, int capacity, std::vector<long long>& first, std::vector<double>& nd,
                        std::vector<int32_t>& dwell, std::vector<double>& rows) {
  first.resize(S), nd.resize(S), dwell.resize(S);
  const long long count = fb::count_rows(t.data(), stop.data(), S, dt, insert, first.data(), nd.data(), dwell.data());
  const long long n = count < capacity ? count : capacity;
  rows.assign((size_t)n * 4, 0.0);
  for (long long r = 0; r < n; ++r) {
    const int i = fb::segment_of_row(first.data(), S, r);
    fb::row_at(&w[(size_t)i * 4], &w[(size_t)i * 4 + 4], fb::row_coeff(nd[i], dwell[i], r - first[i]), &rows[(size_t)r * 4]);
  }
  return count;
}

int main() {
  for (;;) {
    int mode = 0, S = 0, capacity = 0;
    double dt = 0, stopping = 0;
    if (std::scanf("%d", &mode) != 1) return 0;
    if ((mode != 1 && mode != 2) || std::scanf("%d %d %lf %lf", &S, &capacity, &dt, &stopping) != 4 || S < 1) return 2;
    int has_up = 0, relax = 0;
    double speed = 1, accel = 1;
    if (mode == 1 && std::scanf("%d", &has_up) != 1) return 2;
    if (mode == 2 && std::scanf("%d %lf %lf", &relax, &speed, &accel) != 3) return 2;
    std::vector<double> w((size_t)(S + 1) * 4), sf(S + 1), t(S), lim(mode == 2 ? 9 : 0), up;
    if (!read(w) || !read(sf)) return 2;
    if (mode == 1 && !read(t)) return 2;
    if (mode == 2 && !read(lim)) return 2;
    if (has_up) {
      up.resize((size_t)(capacity > 0 ? capacity : 0) * 4);
      if (!read(up)) return 2;
    }
    std::vector<uint8_t> stop(S + 1);
    for (int v = 0; v <= S; ++v) stop[v] = sf[v] != 0.0;
    int32_t insert = 0;
    if (!(dt > 0.0) || !std::isfinite(dt) || !(stopping >= 0.0) || !std::isfinite(stopping) ||
        !fb::insert_count(stopping, dt, &insert) || capacity < 1 || capacity > fb::kMaxCapacity) {
      std::printf("invalid\n");
      continue;
    }
    if (mode == 2) {
      std::vector<double> unwrapped(w.size());
      fb::unwrap_path(w.data(), S + 1, unwrapped.data());
      lim[0] *= speed, lim[1] *= speed, lim[3] *= accel, lim[4] *= accel;
      if (relax) lim[2] = lim[5] = lim[8] = (double)FLT_MAX;
      const bc::Thresholds th = bc::thresholds(lim.data());
      for (int i = 0; i < S; ++i) t[i] = bc::classify(unwrapped.data(), i, S, lim.data(), th).value;
      for (int v = 0; v <= S; ++v) std::printf("%.17g ", unwrapped[(size_t)v * 4 + 3]);
      for (double x : t) std::printf("%.17g ", x);
    }
    std::vector<long long> first;
    std::vector<double> nd, rows;
    std::vector<int32_t> dwell;
    const long long count = sample(w, stop, t, S, dt, insert, capacity, first, nd, dwell, rows);
    std::printf("%lld ", count);
    if (mode == 1) {
      std::printf("%d ", fb::saturated(count, capacity));
      for (int i = 0; i < S; ++i) std::printf("%d ", fb::saturated(first[i], capacity));
    }
    for (double x : rows) std::printf("%.17g ", x);
    if (has_up) {
      const long long n = count < capacity ? count : capacity;
      for (int v = 0; v <= S; ++v) {  // the kernel's walk leaves every vertex these sums
        double g[4];
        fb::vertex_gradient(first.data(), nd.data(), dwell.data(), S, n, up.data(), v, g);
        for (int k = 0; k < 4; ++k) std::printf("%.17g ", g[k]);
      }
    }
    std::printf("\n");
  }
}

// pathedit_harness.cpp -- path thinning, mid-point subdivision and their backward pass (csrc/mrs_tg_pathedit.hpp: the decision,
// the rule, the mid-point and the sums thin_path_kernel, insert_midpoints_kernel, edit_write_kernel and path_edit_vjp_kernel run)
// compiled with plain g++ for the CPU, one path after the other; and the policy layer's own two functions on top of them
// (csrc/mrs_tg_policy_host.hpp).  tests/test_pathedit_host.py checks it against the oracle's mto_preprocess_path and a
// restatement of :739-753 on mto_interpolate_point; tests/test_gpu_pathedit.py checks the kernels against it.
//
//   g++ -std=c++17 -O2 -ffp-contract=off tests/host/pathedit_harness.cpp -o pathedit_harness && ./pathedit_harness < in
//
// Input (whitespace separated), any number of problems until end of input, V >= 1 vertices each:
//   1 V min_distance enabled max_deviation max_hdg_deviation  waypoints [V][4]  stop_at [V]
//     -> one line: n and the kept input indices [n] of the serial loop, n and the kept input indices of the 64-candidate window,
//        n and the kept rows' stop_at [n] and rows [n][4] of policy::preprocess
//   2 V first_segment  waypoints [V][4]  stop_at [V]  unsafe [V - 1]
//     -> one line: n, rows [n][4], stop_at [n], source [n], inserted [n] of pathq::subdivide_path
//   3 n_in n_run has_inserted  source [n_run]  inserted [n_run]  upstream [n_run][4]
//     -> one line: dL/dwaypoints [n_in][4] (pathq::edit_gradient of every input vertex 0 .. n_in - 1)
//   4 V n_samples first_segment max_deviation  waypoints [V][4]  stop_at [V]  samples [n_samples][4]
//     -> one line: is_safe, n, rows [n][4], stop_at [n] of devq::validate + policy::insert_midpoints (inserted when not safe, as
//        the policy loop does)
// Doubles are printed with 17 significant digits: the bits survive.
#include <cstdio>
#include <vector>

#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_pathedit.hpp"
#include "../../mrs_uav_trajectory_generation_amd/csrc/mrs_tg_policy_host.hpp"

namespace pq = mrs_tg::pathq;
namespace pol = mrs_tg::policy;

static bool read(std::vector<double>& v) {
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}
static void print(const std::vector<double>& v, size_t n) {
  for (size_t i = 0; i < n; ++i) std::printf("%.17g ", v[i]);
}

int main() {
  for (;;) {
    int mode = 0;
    if (std::scanf("%d", &mode) != 1) return 0;
    if (mode == 1) {
      int V = 0, enabled = 0;
      pq::ThinOptions o{};
      if (std::scanf("%d %lf %d %lf %lf", &V, &o.min_waypoint_distance, &enabled, &o.straightener_max_deviation,
                     &o.straightener_max_hdg_deviation) != 5 || V < 1)
        return 2;
      o.straightener_enabled = enabled;
      std::vector<double> w((size_t)V * 4), sf(V);
      if (!read(w) || !read(sf)) return 2;
      std::vector<int32_t> kept(V);
      int n = pq::thin_path_serial(w.data(), 4, V, o, kept.data());
      std::printf("%d ", n);
      for (int k = 0; k < n; ++k) std::printf("%d ", kept[k]);
      n = pq::thin_path(w.data(), 4, V, o, kept.data());
      std::printf("%d ", n);
      for (int k = 0; k < n; ++k) std::printf("%d ", kept[k]);
      std::vector<mrs_tg_waypoint> in(V);
      for (int v = 0; v < V; ++v) {
        for (int k = 0; k < 4; ++k) in[v].coords[k] = w[(size_t)v * 4 + k];
        in[v].stop_at = sf[v] != 0.0;
      }
      mrs_tg_policy_options po{};
      po.min_waypoint_distance = o.min_waypoint_distance;
      po.path_straightener_enabled = enabled;
      po.path_straightener_max_deviation = o.straightener_max_deviation;
      po.path_straightener_max_hdg_deviation = o.straightener_max_hdg_deviation;
      pol::PathState st;
      pol::preprocess(in.data(), V, po, st);
      std::printf("%d ", st.n_wp);
      for (int k = 0; k < st.n_wp; ++k) std::printf("%d ", (int)st.stop[k]);
      print(st.wps, (size_t)st.n_wp * 4);
      std::printf("\n");
    } else if (mode == 2) {
      int V = 0, first_segment = 0;
      if (std::scanf("%d %d", &V, &first_segment) != 2 || V < 1) return 2;
      std::vector<double> w((size_t)V * 4), sf(V), uf(V - 1);
      if (!read(w) || !read(sf) || !read(uf)) return 2;
      std::vector<uint8_t> stop(V), unsafe(V > 1 ? V - 1 : 1);
      for (int v = 0; v < V; ++v) stop[v] = sf[v] != 0.0;
      for (int s = 0; s + 1 < V; ++s) unsafe[s] = uf[s] != 0.0;
      const size_t cap = 2 * (size_t)V;
      std::vector<double> out(cap * 4);
      std::vector<uint8_t> stop_out(cap), inserted(cap);
      std::vector<int32_t> source(cap);
      const int n = pq::subdivide_path(w.data(), stop.data(), V, unsafe.data(), first_segment, out.data(), stop_out.data(),
                                       source.data(), inserted.data());
      std::printf("%d ", n);
      print(out, (size_t)n * 4);
      for (int k = 0; k < n; ++k) std::printf("%d ", (int)stop_out[k]);
      for (int k = 0; k < n; ++k) std::printf("%d ", source[k]);
      for (int k = 0; k < n; ++k) std::printf("%d ", (int)inserted[k]);
      std::printf("\n");
    } else if (mode == 3) {
      int n_in = 0, n_run = 0, has_inserted = 0;
      if (std::scanf("%d %d %d", &n_in, &n_run, &has_inserted) != 3 || n_in < 0 || n_run < 0) return 2;
      std::vector<double> sf(n_run), inf(n_run), up((size_t)n_run * 4);
      if (!read(sf) || !read(inf) || !read(up)) return 2;
      std::vector<int32_t> source(n_run + 1);
      std::vector<uint8_t> inserted(n_run + 1);
      for (int k = 0; k < n_run; ++k) source[k] = (int32_t)sf[k], inserted[k] = inf[k] != 0.0;
      for (int v = 0; v < n_in; ++v) {
        double g[4];
        pq::edit_gradient(source.data(), has_inserted ? inserted.data() : nullptr, n_run, v, up.data(), g);
        for (int k = 0; k < 4; ++k) std::printf("%.17g ", g[k]);
      }
      std::printf("\n");
    } else if (mode == 4) {
      int V = 0, n = 0, first_segment = 0;
      mrs_tg_policy_options po{};
      if (std::scanf("%d %d %d %lf", &V, &n, &first_segment, &po.max_deviation) != 4 || V < 1 || n < 0) return 2;
      po.max_deviation_first_segment = first_segment;
      po.check_deviation_enabled = 1;
      pol::PathState st;
      st.wps.resize((size_t)V * 4);
      std::vector<double> sf(V), samples((size_t)n * 4);
      if (!read(st.wps) || !read(sf) || !read(samples)) return 2;
      st.stop.resize(V);
      for (int v = 0; v < V; ++v) st.stop[v] = sf[v] != 0.0;
      st.n_wp = V;
      std::vector<uint8_t> safe;
      double max_dev = 0.0;
      const bool is_safe = pol::validate_spatial(samples.data(), n, st, po, safe, max_dev);
      if (!is_safe) pol::insert_midpoints(st, safe, po);
      std::printf("%d %d ", (int)is_safe, st.n_wp);
      print(st.wps, (size_t)st.n_wp * 4);
      for (int k = 0; k < st.n_wp; ++k) std::printf("%d ", (int)st.stop[k]);
      std::printf("\n");
    } else {
      return 2;
    }
  }
}

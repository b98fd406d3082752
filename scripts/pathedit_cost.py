#!/usr/bin/env python3
"""What the two path-edit steps and their backward pass cost: mrs_tg_plan_preprocess_path (thin_path_kernel,
vertex_offsets_kernel, edit_write_kernel), mrs_tg_plan_insert_midpoints (insert_midpoints_kernel, vertex_offsets_kernel,
edit_write_kernel) and mrs_tg_plan_path_edit_vjp (path_edit_vjp_kernel) on the GPU, each per CALL from the library's own events
(kernel ids 20, 21, 22; the two forward calls from the start of their first launch to the end of their third), beside the policy
layer's host functions on the same batch: policy::preprocess and policy::insert_midpoints of csrc/mrs_tg_policy_host.hpp,
compiled here with g++ -O2 and run on ONE thread (mrs_tg_optimize_paths spreads them over up to 16).

    python scripts/pathedit_cost.py [--reps 30] [--configs 1024x10,10240x10]

Random paths at the bench's limits; every fourth vertex sits within min_waypoint_distance of the one before it, every second
segment is reported unsafe.  What a device-resident caller saves beside these times is not in them: the two copies of the
waypoints per round.  Prints one JSON line per configuration, medians in microseconds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402

HOST_PROGRAM = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "mrs_uav_trajectory_generation_amd/csrc/mrs_tg_policy_host.hpp"
namespace pol = mrs_tg::policy;
int main(int argc, char** argv) {
  int P = 0, V = 0, reps = 0;
  double min_distance = 0;
  if (std::scanf("%d %d %d %lf", &P, &V, &reps, &min_distance) != 4) return 2;
  std::vector<mrs_tg_waypoint> in((size_t)P * V);
  std::vector<uint8_t> safe((size_t)P * (V - 1));
  for (auto& w : in) {
    if (std::scanf("%lf %lf %lf %lf", &w.coords[0], &w.coords[1], &w.coords[2], &w.coords[3]) != 4) return 2;
    w.stop_at = 0;
  }
  for (auto& s : safe) {
    int v = 0;
    if (std::scanf("%d", &v) != 1) return 2;
    s = (uint8_t)v;
  }
  mrs_tg_policy_options o{};
  o.min_waypoint_distance = min_distance;
  o.max_deviation_first_segment = 1;
  std::vector<pol::PathState> st(P), work(P);
  std::vector<std::vector<uint8_t>> flags(P);
  for (int p = 0; p < P; ++p) flags[p].assign(safe.begin() + (size_t)p * (V - 1), safe.begin() + (size_t)(p + 1) * (V - 1));
  for (int r = 0; r < reps; ++r) {
    auto t0 = std::chrono::steady_clock::now();
    for (int p = 0; p < P; ++p) pol::preprocess(in.data() + (size_t)p * V, V, o, st[p]);
    auto t1 = std::chrono::steady_clock::now();
    for (int p = 0; p < P; ++p) {   // the untouched path, as the second round would see it
      work[p].wps.resize((size_t)V * 4);
      for (int v = 0; v < V; ++v)
        for (int k = 0; k < 4; ++k) work[p].wps[(size_t)v * 4 + k] = in[(size_t)p * V + v].coords[k];
      work[p].stop.assign(V, 0);
      work[p].n_wp = V;
    }
    auto t2 = std::chrono::steady_clock::now();
    for (int p = 0; p < P; ++p) pol::insert_midpoints(work[p], flags[p], o);
    auto t3 = std::chrono::steady_clock::now();
    std::printf("%.3f %.3f\n", std::chrono::duration<double, std::micro>(t1 - t0).count(),
                std::chrono::duration<double, std::micro>(t3 - t2).count());
  }
  long long kept = 0, grown = 0;
  for (int p = 0; p < P; ++p) kept += st[p].n_wp, grown += work[p].n_wp;
  std::printf("%lld %lld\n", kept, grown);
}
"""


def host_times(wp, unsafe, P, V, reps, min_distance):
    """-> (median us of preprocess, median us of insert_midpoints, vertices kept, vertices after subdivision)"""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "host.cpp"), os.path.join(tmp, "host")
        with open(src, "w") as f:
            f.write(HOST_PROGRAM)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", ROOT, src, "-o", exe, "-pthread"], check=True)
        text = "%d %d %d %r\n" % (P, V, reps, min_distance)
        text += "\n".join(" ".join(repr(float(x)) for x in row) for row in wp) + "\n"
        text += " ".join(str(int(not u)) for u in unsafe) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    t = np.array([[float(x) for x in line.split()] for line in out[:reps]])
    kept, grown = (int(x) for x in out[reps].split())
    return float(np.median(t[:, 0])), float(np.median(t[:, 1])), kept, grown


def measure(ctx, n_paths, n_seg, reps):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    so = np.asarray(batch.seg_offsets)
    P, nS = batch.n_paths, batch.n_segments
    nV, V = nS + P, n_seg + 1
    min_distance, max_deviation = 0.05, 0.05
    wp = np.array(batch.waypoints, dtype=np.float64)
    rng = np.random.default_rng(0)
    local = np.arange(nV) - np.repeat(so[:-1] + np.arange(P), V)
    near = (local % 4 == 2) & (local < V - 1)
    wp[near, :3] = wp[np.flatnonzero(near) - 1, :3] + rng.uniform(-0.01, 0.01, size=(int(near.sum()), 3))
    unsafe = (np.arange(nS) % 2 == 0)
    seg_max = np.where(unsafe, 2.0 * max_deviation, 0.5 * max_deviation)
    plan = api.Plan(ctx, so)
    f64, i32, u8 = (dict(dtype=t, device="cuda") for t in (torch.float64, torch.int32, torch.uint8))
    d_wp, d_seg_max = torch.from_numpy(wp).cuda(), torch.from_numpy(seg_max).cuda()
    offsets = torch.empty(P + 1, **i32)
    rows, stop, source, inserted = torch.empty((nV + nS, 4), **f64), torch.empty(nV + nS, **u8), torch.empty(nV + nS, **i32), \
        torch.empty(nV + nS, **u8)
    grad_in = torch.empty((nV, 4), **f64)
    out = OrderedDict((k, []) for k in ("preprocess_path", "insert_midpoints", "path_edit_vjp"))
    ctx.set_profiling(True)
    for r in range(reps + 2):
        plan.preprocess_path(d_wp, offsets, rows, min_waypoint_distance=min_distance, stop_at_out=stop, source=source)
        t_thin = ctx.kernel_ms_history(api.KERNEL_PREPROCESS_PATH, 1)[-1:]
        kept = int(offsets[-1].item())
        plan.insert_midpoints(d_wp, d_seg_max, max_deviation, offsets, rows, stop_at_out=stop, source=source, inserted=inserted)
        t_sub = ctx.kernel_ms_history(api.KERNEL_INSERT_MIDPOINTS, 1)[-1:]
        grown = int(offsets[-1].item())
        grad = torch.ones((grown, 4), **f64)
        plan.path_edit_vjp(offsets, source, grad, grad_in, inserted=inserted)
        t_vjp = ctx.kernel_ms_history(api.KERNEL_PATH_EDIT_VJP, 1)[-1:]
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["preprocess_path"] += t_thin
            out["insert_midpoints"] += t_sub
            out["path_edit_vjp"] += t_vjp
    ctx.set_profiling(False)
    plan.close()
    h_thin, h_sub, h_kept, h_grown = host_times(wp, unsafe, P, V, reps, min_distance)
    assert (h_kept, h_grown) == (kept, grown), (h_kept, kept, h_grown, grown)      # the same batch, the same decisions
    res = OrderedDict(config="%dx%d" % (n_paths, n_seg), vertices=nV, vertices_kept=kept, vertices_subdivided=grown, reps=reps)
    for k, v in out.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e3, 2)
    res["host_preprocess_one_thread_us"] = round(h_thin, 1)
    res["host_insert_midpoints_one_thread_us"] = round(h_sub, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="1024x10,10240x10")
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        n, s = cfg.split("x")
        print(json.dumps(measure(ctx, int(n), int(s), a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

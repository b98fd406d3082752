#!/usr/bin/env python3
"""What the segment-time estimate as a plan step and its backward pass cost: estimate_times_kernel
(mrs_tg_plan_estimate_times) and estimate_times_vjp_kernel (mrs_tg_plan_estimate_times_vjp) on the GPU, beside the traffic
neither can avoid.

    python scripts/estimate_cost.py [--reps 30] [--configs 10240x10,65536x10]

Per configuration, alternating within the run: the forward; the backward pass with all three outputs; the backward pass with
the waypoint gradient alone; the terms alone (no upstream).  All are timed by the library's own per-dispatch events (kernel ids
10 and 11).  The compulsory traffic: the forward reads 32 B per vertex and 72 B per path and writes 8 B per segment; the
backward pass reads 32 B per vertex, 8 B per segment and 72 B per path and writes 32 B per vertex, 4 B per segment (the term)
and 72 B per path.  Prints one JSON line per configuration: medians in microseconds, the bytes, the bandwidth they would mean
and the ratio of the backward pass to the forward.  Both kernels are a few microseconds long at these sizes: what is measured
is the cost of a launch more than that of the traffic.
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402


def measure(ctx, n_paths, n_seg, reps):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    nS, P = batch.n_segments, batch.n_paths
    nV = nS + P
    wp = torch.from_numpy(batch.waypoints).cuda()
    lim = torch.from_numpy(batch.limits).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    G = torch.randn(nS, dtype=torch.float64, device="cuda", generator=gen)
    times = torch.empty(nS, dtype=torch.float64, device="cuda")
    gw, gl = torch.empty_like(wp), torch.empty_like(lim)
    term = torch.empty(nS, dtype=torch.int32, device="cuda")
    out = OrderedDict((k, []) for k in ("forward", "vjp", "vjp_waypoints_only", "terms_only"))

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["forward"] = timed(api.KERNEL_ESTIMATE, lambda: plan.estimate_times(wp, lim, times))
        got["vjp"] = timed(api.KERNEL_ESTIMATE_VJP, lambda: plan.estimate_times_vjp(wp, lim, G, grad_waypoints=gw, grad_limits=gl,
                                                                                 term=term))
        got["vjp_waypoints_only"] = timed(api.KERNEL_ESTIMATE_VJP, lambda: plan.estimate_times_vjp(wp, lim, G, grad_waypoints=gw))
        got["terms_only"] = timed(api.KERNEL_ESTIMATE_VJP, lambda: plan.estimate_times_vjp(wp, lim, term=term))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            for k, v in got.items():
                out[k] += v
    hist = torch.bincount(term.to(torch.int64), minlength=4).cpu().tolist()
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    fwd_bytes = 32 * nV + 72 * P + 8 * nS
    vjp_bytes = (32 + 32) * nV + (8 + 4) * nS + (72 + 72) * P
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, vertices=nV, reps=reps,
                      terms=dict(horizontal=hist[0], vertical=hist[1], floor=hist[2], heading=hist[3]))
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["forward_bytes"], res["vjp_bytes"] = fwd_bytes, vjp_bytes
    res["forward_GBps"] = round(fwd_bytes / med["forward"] * 1e-3, 1)
    res["vjp_GBps"] = round(vjp_bytes / med["vjp"] * 1e-3, 1)
    res["vjp_over_forward"] = round(med["vjp"] / med["forward"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="10240x10,65536x10")
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        n, s = cfg.split("x")
        print(json.dumps(measure(ctx, int(n), s if s == "ragged" else int(s), a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

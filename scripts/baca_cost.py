#!/usr/bin/env python3
"""What the Baca segment-time estimate as a plan step, its backward pass and the length gate cost: baca_times_kernel
(mrs_tg_plan_estimate_times_baca), baca_times_vjp_kernel (mrs_tg_plan_estimate_times_baca_vjp) and length_gate_kernel
(mrs_tg_plan_length_gate) on the GPU, beside the Euclidean pair measured in the same run as the yardsticks:
estimate_times_kernel (mrs_tg_plan_estimate_times) and estimate_times_vjp_kernel (mrs_tg_plan_estimate_times_vjp).

    python scripts/baca_cost.py [--reps 30] [--configs 10240x10,65536x10]

Per configuration, alternating within the run: both forwards; both backward passes with all three outputs; the Baca backward
pass with the waypoint gradient alone and with the flags alone (no upstream); the gate.  All are timed by the library's own
per-dispatch events (kernel ids 10, 11, 14, 15, 16).  The compulsory traffic: either forward reads 32 B per vertex and 72 B per
path and writes 8 B per segment; either backward pass reads 32 B per vertex, 8 B per segment and 72 B per path and writes 32 B
per vertex, 4 B per segment and 72 B per path; the gate reads 8 B per segment and 8 B per path and writes 12 B per path.
Prints one JSON line per configuration: medians in microseconds, the bytes, and the ratios of each Baca kernel to its
Euclidean yardstick.  The backward pass recomputes four segments per vertex lane where the Euclidean one recomputes two.
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
    flags = torch.empty(nS, dtype=torch.int32, device="cuda")
    n_samples = torch.full((P,), 100, dtype=torch.int32, device="cuda")
    status = torch.ones(P, dtype=torch.int32, device="cuda")
    total = torch.empty(P, dtype=torch.float64, device="cuda")
    verdict = torch.empty(P, dtype=torch.int32, device="cuda")
    out = OrderedDict((k, []) for k in ("euclid_forward", "baca_forward", "euclid_vjp", "baca_vjp", "baca_vjp_waypoints_only",
                                        "baca_flags_only", "length_gate"))

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["euclid_forward"] = timed(api.KERNEL_ESTIMATE, lambda: plan.estimate_times(wp, lim, times))
        got["baca_forward"] = timed(api.KERNEL_BACA, lambda: plan.estimate_times_baca(wp, lim, times))
        got["euclid_vjp"] = timed(api.KERNEL_ESTIMATE_VJP, lambda: plan.estimate_times_vjp(wp, lim, G, grad_waypoints=gw,
                                                                                        grad_limits=gl, term=term))
        got["baca_vjp"] = timed(api.KERNEL_BACA_VJP, lambda: plan.estimate_times_baca_vjp(wp, lim, G, grad_waypoints=gw,
                                                                                         grad_limits=gl, flags=flags))
        got["baca_vjp_waypoints_only"] = timed(api.KERNEL_BACA_VJP,
                                               lambda: plan.estimate_times_baca_vjp(wp, lim, G, grad_waypoints=gw))
        got["baca_flags_only"] = timed(api.KERNEL_BACA_VJP, lambda: plan.estimate_times_baca_vjp(wp, lim, flags=flags))
        got["length_gate"] = timed(api.KERNEL_LENGTH_GATE, lambda: plan.length_gate(times, n_samples, 0.2, 3.0, 0.33, status=status,
                                                                                   total=total, verdict=verdict))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            for k, v in got.items():
                out[k] += v
    f = flags.to(torch.int64)
    hist = OrderedDict((name, int(((f & bit) != 0).sum())) for name, bit in (
        ("v_vertical", 1), ("a_vertical", 2), ("j_vertical", 4), ("t1_capped", 8), ("t2_capped", 16), ("dot1_clamped", 32),
        ("dot2_clamped", 64), ("floor", 128), ("heading", 256)))
    verdicts = torch.bincount(verdict.to(torch.int64), minlength=4).cpu().tolist()
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    fwd_bytes = 32 * nV + 72 * P + 8 * nS
    vjp_bytes = (32 + 32) * nV + (8 + 4) * nS + (72 + 72) * P
    gate_bytes = 8 * nS + (4 + 4 + 8 + 4) * P
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, vertices=nV, reps=reps, flags=hist, verdicts=verdicts)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["forward_bytes"], res["vjp_bytes"], res["gate_bytes"] = fwd_bytes, vjp_bytes, gate_bytes
    res["baca_forward_GBps"] = round(fwd_bytes / med["baca_forward"] * 1e-3, 1)
    res["baca_vjp_GBps"] = round(vjp_bytes / med["baca_vjp"] * 1e-3, 1)
    res["baca_forward_over_euclid_forward"] = round(med["baca_forward"] / med["euclid_forward"], 2)
    res["baca_vjp_over_euclid_vjp"] = round(med["baca_vjp"] / med["euclid_vjp"], 2)
    res["baca_vjp_over_baca_forward"] = round(med["baca_vjp"] / med["baca_forward"], 2)
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

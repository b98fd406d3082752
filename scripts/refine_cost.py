#!/usr/bin/env python3
"""What MRS_TG_FLAG_REFINE costs: the fixed-times solve of Plan.solve with and without the flag, alternating, on the GPU.

    python scripts/refine_cost.py [--reps 50] [--configs 1024x10,10240x10,65536x10,8192xragged]

Per configuration the batch's times come from the library's estimator (one solve with estimate_times), then the default solve
is timed with torch events around each call, the two variants interleaved so that clocks and placement drift affect both
alike.  Prints one JSON line per configuration: medians in microseconds of the call without the flag, with it, and their
difference (the refine kernel's share; under `rocprofv3 --kernel-trace --stats -- python scripts/refine_cost.py` the kernel
statistics give the dispatch times of solve and refine kernels separately).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402


def measure(ctx, n_paths, n_seg, reps):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    opts = {False: api.default_options(derivative_to_optimize=4),
            True: api.default_options(derivative_to_optimize=4, flags=api.FLAG_REFINE)}
    kernels = {k: plan.explain(o) for k, o in opts.items()}
    times = {False: [], True: []}
    for r in range(reps + 2):
        for flag in ((False, True) if r % 2 == 0 else (True, False)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            plan.solve(opts[flag], db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost)
            b.record()
            torch.cuda.synchronize()
            if r >= 2:   # (the first two rounds: allocation of the refine workspace, code upload)
                times[flag].append(a.elapsed_time(b) * 1e3)
    plan.close()
    plain, ref = float(np.median(times[False])), float(np.median(times[True]))
    return dict(config="%dx%s" % (n_paths, n_seg), reps=reps, solve_us=round(plain, 2), solve_refine_us=round(ref, 2),
                refine_share_us=round(ref - plain, 2), ratio=round(ref / plain, 2), kernels_plain=kernels[False],
                kernels_refine=kernels[True])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--configs", default="1024x10,10240x10,65536x10,8192xragged")
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        n, s = cfg.split("x")
        print(json.dumps(measure(ctx, int(n), s if s == "ragged" else int(s), a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

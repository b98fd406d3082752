#!/usr/bin/env python3
"""What the backward pass of the segment maxima costs: segment_maxima_vjp_kernel (mrs_tg_plan_segment_maxima_vjp) against the
forward segment_maxima9_kernel (mrs_tg_plan_segment_maxima) it differentiates, on the GPU.

    python scripts/maxima_vjp_cost.py [--reps 50] [--configs 1024x10,10240x10,65536x10,8192xragged]
    python scripts/maxima_vjp_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                            rocprofv3 --kernel-trace --stats run of the line above)

Per configuration the batch's times come from the library's estimator (one solve with estimate_times) and its coefficients
from the default fixed-times solve; then, alternating within the run, the forward maxima and the backward pass with all nine
upstream entries of every segment non-zero (all outputs: coefficient and time gradients and t*).  The backward dispatch is
timed by the library's own per-dispatch events (kernel id 4); the forward launch is not a timed family, so its line gives torch
events around the call (launch included) -- the rocprofv3 summary is the like-for-like kernel comparison.  Prints one JSON
line per configuration: medians in microseconds and their ratio.
"""
import argparse
import csv
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
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    plan.solve(api.default_options(derivative_to_optimize=4), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status,
               db.cost)
    nS = batch.n_segments
    rng = np.random.default_rng(0)
    G = rng.standard_normal((nS, 3, 3))
    G[G == 0.0] = 1.0
    G = torch.from_numpy(G).cuda()
    maxima = torch.empty((nS, 3, 3), dtype=torch.float64, device="cuda")
    gc = torch.empty((nS, 4, 10), dtype=torch.float64, device="cuda")
    gt = torch.empty(nS, dtype=torch.float64, device="cuda")
    am = torch.empty((nS, 3, 3), dtype=torch.float64, device="cuda")
    out = {"forward": [], "vjp": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(reps + 2):
        e0.record()
        plan.segment_maxima(db.coeffs, db.seg_times, maxima)
        e1.record()
        ctx.set_profiling(True)
        plan.segment_maxima_vjp(db.coeffs, db.seg_times, G, gc, gt, am)
        b = ctx.kernel_ms_history(api.KERNEL_MAXIMA_VJP, 1)
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["forward"].append(e0.elapsed_time(e1))
            out["vjp"] += b
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    return OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, reps=reps, forward_event_us=round(med["forward"], 2),
                       vjp_us=round(med["vjp"], 2), vjp_over_forward=round(med["vjp"] / med["forward"], 2))


def _trace_rows(path):
    """kernel dispatches of a rocprofv3 --kernel-trace run: its CSV (--output-format csv) or its rocpd database (the default)"""
    if path.endswith(".db"):
        import sqlite3
        cur = sqlite3.connect(path).execute("select name, grid_x, workgroup_x, start, end, vgpr_count, accum_vgpr_count, sgpr_count, "
                                            "scratch_size from kernels order by start")
        return [dict(Kernel_Name=r[0], Grid_Size_X=str(r[1]), Workgroup_Size_X=str(r[2]), Start_Timestamp=r[3], End_Timestamp=r[4],
                     VGPR_Count=str(r[5]), Accum_VGPR_Count=str(r[6]), SGPR_Count=str(r[7]), Scratch_Size=str(r[8])) for r in cur]
    return list(csv.DictReader(open(path)))


def summarize(path):
    """kernel trace -> per kernel name (in order of first appearance) and grid: dispatches, median / min / max us, registers"""
    rows = _trace_rows(path)
    groups = OrderedDict()
    for r in rows:
        name = r.get("Kernel_Name", "").replace("void ", "").replace("mrs_tg::", "").split("(")[0]
        if "maxima" not in name:
            continue
        key = (name, r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", "")))
        g = groups.setdefault(key, dict(t=[], vgpr=r.get("VGPR_Count", r.get("Arch_VGPR_Count", "")),
                                        agpr=r.get("Accum_VGPR_Count", ""), sgpr=r.get("SGPR_Count", ""),
                                        scratch=r.get("Scratch_Size", r.get("Private_Segment_Size", ""))))
        g["t"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# kernel                           grid_x   wg    n  median_us     min_us     max_us  vgpr agpr sgpr scratch")
    for (name, grid, wg), g in groups.items():
        t = np.array(g["t"])
        print("  %-32s %7s %4s %4d %10.2f %10.2f %10.2f  %4s %4s %4s %s" % (name[:32], grid, wg, t.size, np.median(t), t.min(), t.max(),
                                                                          g["vgpr"], g["agpr"], g["sgpr"], g["scratch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--configs", default="1024x10,10240x10,65536x10,8192xragged")
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
        return
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        n, s = cfg.split("x")
        print(json.dumps(measure(ctx, int(n), s if s == "ragged" else int(s), a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the backward pass of the fixed-times solve costs: vjp_kernel (mrs_tg_plan_solve_vjp) against the forward solve it
differentiates, on the GPU.

    python scripts/vjp_cost.py [--reps 50] [--configs 1024x10,10240x10,65536x10,8192xragged]
    python scripts/vjp_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                     rocprofv3 --kernel-trace --stats run of the line above)

Per configuration the batch's times come from the library's estimator (one solve with estimate_times); then, alternating, the
default fixed-times solve (the flagship's kernel), the general-pattern solve that autograd.solve runs, and the backward pass
with upstream gradients for coefficients and cost, each dispatch timed by the library's own per-dispatch events
(mrs_tg_kernel_ms_history, kernel ids 1 and 3).  Prints one JSON line per configuration: medians in microseconds, the ratio of
the backward pass to the default solve, and the backward pass's workspace (bytes, and bytes per path per vertex).
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

WS_DOUBLES_PER_LANE_VERTEX = 45   # L (15), W (25), z (5): mrs_tg_vjp.hpp kWsPerVertex


def measure(ctx, n_paths, n_seg, reps):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    rng = np.random.default_rng(0)
    G = torch.from_numpy(rng.standard_normal((batch.n_segments, 4, 10))).cuda()
    g = torch.from_numpy(rng.standard_normal(batch.n_paths)).cuda()
    gv, gt = torch.zeros_like(db.fixed_values), torch.zeros_like(db.seg_times)
    plain = api.default_options(derivative_to_optimize=4)
    general = api.default_options(derivative_to_optimize=4, flags=api.FLAG_GENERAL_PATTERNS)
    kernels = dict(solve=plan.explain(plain), solve_general=plan.explain(general))
    out = {"solve": [], "solve_general": [], "vjp": []}
    for r in range(reps + 2):
        ctx.set_profiling(True)
        plan.solve(plain, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost)
        a = ctx.kernel_ms_history(api.KERNEL_SOLVE_LINEAR, 1)
        plan.solve(general, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost)
        b = ctx.kernel_ms_history(api.KERNEL_SOLVE_LINEAR, 1)
        plan.solve_vjp(4, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, G, g, gv, gt)
        c = ctx.kernel_ms_history(api.KERNEL_VJP, 1)
        ctx.set_profiling(False)
        if r >= 2:   # (the first two rounds: workspace allocation, code upload)
            out["solve"] += a
            out["solve_general"] += b
            out["vjp"] += c
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    V = int(np.max(np.diff(batch.seg_offsets))) + 1
    ws = V * WS_DOUBLES_PER_LANE_VERTEX * 4 * 8 * batch.n_paths
    return OrderedDict(config="%dx%s" % (n_paths, n_seg), reps=reps, solve_us=round(med["solve"], 2),
                       solve_general_us=round(med["solve_general"], 2), vjp_us=round(med["vjp"], 2),
                       vjp_over_solve=round(med["vjp"] / med["solve"], 2), workspace_bytes=ws,
                       workspace_bytes_per_path_vertex=WS_DOUBLES_PER_LANE_VERTEX * 4 * 8, kernels=kernels)


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
        if not any(k in name for k in ("solve", "vjp")):
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

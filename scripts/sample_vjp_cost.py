#!/usr/bin/env python3
"""What the backward pass of the sampler costs: sample_vjp_kernel (mrs_tg_plan_sample_states_vjp) against the forward kernels
it differentiates -- sample_kernel<4> (mrs_tg_plan_sample_states) for n_orders = 5, sample_kernel<0> (mrs_tg_plan_sample) for
n_orders = 1 -- on the GPU.

    python scripts/sample_vjp_cost.py [--reps 30] [--dt 0.2] [--configs 1024x10,10240x10,65536x10,8192xragged]
    python scripts/sample_vjp_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                            rocprofv3 --kernel-trace --stats run of the line above;
                                                            counters, if wanted, in a separate --pmc pass with the
                                                            kernel trace only)

Per configuration the batch's times come from the library's estimator (one solve with estimate_times) and its coefficients
from the default fixed-times solve; the capacity is the batch's largest sample count.  Then, alternating within the run, the
two forward samplers and the backward pass for both n_orders (outputs: coefficient and time gradients; Gaussian upstream).
The backward dispatch is timed by the library's own per-dispatch events (kernel id 5); the forward launches are not a timed
family, so their figures are torch events around the call (launch included) -- the rocprofv3 summary is the like-for-like
kernel comparison.  Prints one JSON line per configuration: medians in microseconds and their ratios.
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


def measure(ctx, n_paths, n_seg, reps, dt):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    plan.solve(api.default_options(derivative_to_optimize=4), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status,
               db.cost)
    nS, P = batch.n_segments, batch.n_paths
    n_dev = torch.zeros(P, dtype=torch.int32, device="cuda")
    plan.sample(db.coeffs, db.seg_times, dt, 0, n_dev, None)   # (counts only need no buffer: capacity + 1 = 1 everywhere)
    plan.sample_states_vjp(db.coeffs, db.seg_times, dt, 1 << 20, None, n_samples=n_dev)
    torch.cuda.synchronize()
    cap = int(n_dev.max().item())
    total = int(n_dev.sum().item())
    gen = torch.Generator(device="cuda").manual_seed(0)
    G5 = torch.randn((P, cap, 5, 4), dtype=torch.float64, device="cuda", generator=gen)
    G1 = G5[:, :, 0].contiguous()
    states = torch.empty((P, cap, 5, 4), dtype=torch.float64, device="cuda")
    samples = torch.empty((P, cap, 4), dtype=torch.float64, device="cuda")
    gc = torch.empty((nS, 4, 10), dtype=torch.float64, device="cuda")
    gt = torch.empty(nS, dtype=torch.float64, device="cuda")
    out = {"fwd5": [], "fwd1": [], "vjp5": [], "vjp1": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for r in range(reps + 2):
        ev[0].record()
        plan.sample_states(db.coeffs, db.seg_times, dt, cap, n_dev, states)
        ev[1].record()
        ev[2].record()
        plan.sample(db.coeffs, db.seg_times, dt, cap, n_dev, samples)
        ev[3].record()
        ctx.set_profiling(True)
        plan.sample_states_vjp(db.coeffs, db.seg_times, dt, cap, G5, status=db.status, grad_coeffs=gc, grad_seg_times=gt)
        b5 = ctx.kernel_ms_history(api.KERNEL_SAMPLE_VJP, 1)
        plan.sample_states_vjp(db.coeffs, db.seg_times, dt, cap, G1, status=db.status, grad_coeffs=gc, grad_seg_times=gt)
        b1 = ctx.kernel_ms_history(api.KERNEL_SAMPLE_VJP, 1)
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["fwd5"].append(ev[0].elapsed_time(ev[1]))
            out["fwd1"].append(ev[2].elapsed_time(ev[3]))
            out["vjp5"] += b5[-1:]
            out["vjp1"] += b1[-1:]
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    return OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, samples=total, capacity=cap, dt=dt, reps=reps,
                       forward5_event_us=round(med["fwd5"], 2), vjp5_us=round(med["vjp5"], 2),
                       vjp5_over_forward5=round(med["vjp5"] / med["fwd5"], 2),
                       forward1_event_us=round(med["fwd1"], 2), vjp1_us=round(med["vjp1"], 2),
                       vjp1_over_forward1=round(med["vjp1"] / med["fwd1"], 2))


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
        if "sample" not in name:
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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dt", type=float, default=0.2)
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
        print(json.dumps(measure(ctx, int(n), s if s == "ragged" else int(s), a.reps, a.dt)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

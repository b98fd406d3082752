#!/usr/bin/env python3
"""What the evaluation at caller-given times and its backward pass cost: evaluate_kernel (mrs_tg_plan_evaluate) and
evaluate_vjp_kernel (mrs_tg_plan_evaluate_vjp) against the sampler's kernels doing the same work -- sample_kernel<4> /
sample_kernel<0> (mrs_tg_plan_sample_states / mrs_tg_plan_sample) and sample_vjp_kernel<5> / <1> -- on the GPU.

    python scripts/evaluate_cost.py [--reps 30] [--dt 0.2] [--configs 1024x10,10240x10,65536x10,8192xragged]
    python scripts/evaluate_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                          rocprofv3 --kernel-trace --stats run of the line above;
                                                          counters, if wanted, in a separate --pmc pass with the
                                                          kernel trace only)

Per configuration the batch's times come from the library's estimator (one solve with estimate_times) and its coefficients
from the default fixed-times solve.  The queries are the sampler's own times -- path p is asked at the k-fold repeated
addition of dt for k below its sample count, NaN beyond -- so both routes do the same work; then once more with every path's
queries (and upstream rows) shuffled.  Alternating within the run, in this order (the order --summarize relies on to tell
the variants of one kernel apart):
    sample_kernel<4>, sample_kernel<0>, sample_vjp_kernel<5>, sample_vjp_kernel<1>,
    evaluate_kernel<5>, evaluate_kernel<1>, evaluate_vjp_kernel<5>, evaluate_vjp_kernel<1>      (sorted; dL/dc and dL/dT)
    evaluate_vjp_kernel<5> with dL/dt as well                                                   (sorted)
    evaluate_kernel<5>, evaluate_kernel<1>, evaluate_vjp_kernel<5>, evaluate_vjp_kernel<1>      (shuffled; dL/dc and dL/dT)
The timed families (kernel ids 5, 6, 7) are timed by the library's own per-dispatch events; the forward samplers are not a
timed family, so their figures are torch events around the call (launch included) -- the rocprofv3 summary is the
like-for-like kernel comparison.  Prints one JSON line per configuration: medians in microseconds and the ratios.
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

# how many variants of one kernel a round of measure() launches, in launch order
VARIANTS = {"evaluate_kernel<5>": ("sorted", "shuffled"), "evaluate_kernel<1>": ("sorted", "shuffled"),
            "evaluate_vjp_kernel<5>": ("sorted", "sorted+dt", "shuffled"), "evaluate_vjp_kernel<1>": ("sorted", "shuffled")}


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
    plan.sample_states_vjp(db.coeffs, db.seg_times, dt, 1 << 20, None, n_samples=n_dev)
    torch.cuda.synchronize()
    cap = int(n_dev.max().item())
    total = int(n_dev.sum().item())
    A = np.zeros(cap)
    for k in range(1, cap):
        A[k] = A[k - 1] + dt
    has = torch.arange(cap, device="cuda")[None, :] < n_dev[:, None]
    q = torch.where(has, torch.from_numpy(A).cuda()[None, :], torch.full((), float("nan"), dtype=torch.float64, device="cuda"))
    q = q.contiguous()
    gen = torch.Generator(device="cuda").manual_seed(0)
    G5 = torch.randn((P, cap, 5, 4), dtype=torch.float64, device="cuda", generator=gen)
    G1 = G5[:, :, 0].contiguous()
    perm = torch.rand((P, cap), device="cuda", generator=gen).argsort(dim=1)
    rows = torch.arange(P, device="cuda")[:, None]
    q_sh, G5_sh = q.gather(1, perm).contiguous(), G5[rows, perm].contiguous()
    G1_sh = G5_sh[:, :, 0].contiguous()
    states = torch.empty((P, cap, 5, 4), dtype=torch.float64, device="cuda")
    samples = torch.empty((P, cap, 4), dtype=torch.float64, device="cuda")
    gc = torch.empty((nS, 4, 10), dtype=torch.float64, device="cuda")
    gt = torch.empty(nS, dtype=torch.float64, device="cuda")
    gq = torch.empty((P, cap), dtype=torch.float64, device="cuda")
    out = OrderedDict((k, []) for k in ("fwd5", "fwd1", "svjp5", "svjp1", "ev5", "ev1", "evjp5", "evjp1", "evjp5_dt", "ev5_sh",
                                        "ev1_sh", "evjp5_sh", "evjp1_sh"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ev[0].record()
        plan.sample_states(db.coeffs, db.seg_times, dt, cap, n_dev, states)
        ev[1].record()
        ev[2].record()
        plan.sample(db.coeffs, db.seg_times, dt, cap, n_dev, samples)
        ev[3].record()
        ctx.set_profiling(True)
        c, t, st = db.coeffs, db.seg_times, db.status
        got = OrderedDict()
        got["svjp5"] = timed(api.KERNEL_SAMPLE_VJP, lambda: plan.sample_states_vjp(c, t, dt, cap, G5, status=st, grad_coeffs=gc, grad_seg_times=gt))
        got["svjp1"] = timed(api.KERNEL_SAMPLE_VJP, lambda: plan.sample_states_vjp(c, t, dt, cap, G1, status=st, grad_coeffs=gc, grad_seg_times=gt))
        got["ev5"] = timed(api.KERNEL_EVALUATE, lambda: plan.evaluate(c, t, q, states))
        got["ev1"] = timed(api.KERNEL_EVALUATE, lambda: plan.evaluate(c, t, q, samples))
        got["evjp5"] = timed(api.KERNEL_EVALUATE_VJP, lambda: plan.evaluate_vjp(c, t, q, G5, status=st, grad_coeffs=gc, grad_seg_times=gt))
        got["evjp1"] = timed(api.KERNEL_EVALUATE_VJP, lambda: plan.evaluate_vjp(c, t, q, G1, status=st, grad_coeffs=gc, grad_seg_times=gt))
        got["evjp5_dt"] = timed(api.KERNEL_EVALUATE_VJP, lambda: plan.evaluate_vjp(c, t, q, G5, status=st, grad_coeffs=gc, grad_seg_times=gt,
                                                                                  grad_query_times=gq))
        got["ev5_sh"] = timed(api.KERNEL_EVALUATE, lambda: plan.evaluate(c, t, q_sh, states))
        got["ev1_sh"] = timed(api.KERNEL_EVALUATE, lambda: plan.evaluate(c, t, q_sh, samples))
        got["evjp5_sh"] = timed(api.KERNEL_EVALUATE_VJP, lambda: plan.evaluate_vjp(c, t, q_sh, G5_sh, status=st, grad_coeffs=gc, grad_seg_times=gt))
        got["evjp1_sh"] = timed(api.KERNEL_EVALUATE_VJP, lambda: plan.evaluate_vjp(c, t, q_sh, G1_sh, status=st, grad_coeffs=gc, grad_seg_times=gt))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["fwd5"].append(ev[0].elapsed_time(ev[1]))
            out["fwd1"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, queries=total, per_path=cap, dt=dt, reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["ev5_over_sample_kernel4_event"] = round(med["ev5"] / med["fwd5"], 2)
    res["ev1_over_sample_kernel0_event"] = round(med["ev1"] / med["fwd1"], 2)
    res["evjp5_over_sample_vjp5"] = round(med["evjp5"] / med["svjp5"], 2)
    res["evjp1_over_sample_vjp1"] = round(med["evjp1"] / med["svjp1"], 2)
    return res


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
    """kernel trace -> per kernel name (in order of first appearance), grid and variant: dispatches, median / min / max us,
    registers.  The variants of one kernel on one grid are told apart by their position in the round (VARIANTS)."""
    rows = sorted(_trace_rows(path), key=lambda r: int(r["Start_Timestamp"]))
    groups = OrderedDict()
    seen = {}
    for r in rows:
        name = r.get("Kernel_Name", "").replace("void ", "").replace("mrs_tg::", "").split("(")[0]
        if "sample" not in name and "evaluate" not in name:
            continue
        grid, wg = r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", ""))
        variants = VARIANTS.get(name, ("",))
        i = seen.get((name, grid), 0)
        seen[(name, grid)] = i + 1
        key = (name, grid, wg, variants[i % len(variants)])
        g = groups.setdefault(key, dict(t=[], vgpr=r.get("VGPR_Count", r.get("Arch_VGPR_Count", "")),
                                        agpr=r.get("Accum_VGPR_Count", ""), sgpr=r.get("SGPR_Count", ""),
                                        scratch=r.get("Scratch_Size", r.get("Private_Segment_Size", ""))))
        g["t"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# kernel                    variant     grid_x   wg    n  median_us     min_us     max_us  vgpr agpr sgpr scratch")
    for (name, grid, wg, variant), g in groups.items():
        t = np.array(g["t"])
        print("  %-25s %-10s %8s %4s %4d %10.2f %10.2f %10.2f  %4s %4s %4s %s" % (name[:25], variant, grid, wg, t.size, np.median(t), t.min(),
                                                                               t.max(), g["vgpr"], g["agpr"], g["sgpr"], g["scratch"]))


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

#!/usr/bin/env python3
"""What the mutual clearance within groups of paths and its backward pass cost: mutual_clearance_kernel
(mrs_tg_plan_mutual_clearance, one workgroup per path, one lane per row, the group's other paths the outer loop) and
mutual_clearance_vjp_kernel (mrs_tg_plan_mutual_clearance_vjp, a gather) against the torch composition that was the only route
before the step existed -- rows -> pairwise differences [G][N][N][Q][3] -> norm -> min over the neighbours, and its autograd
backward -- on the GPU.

    python scripts/clearance_cost.py [--reps 20] [--configs 64x16x512,8x128x512]      (groups x paths per group x rows)

The rows are random walks of 0.1 m steps from starts in a 20 m box, drawn on the device from a seed: every path has all its rows and all paths start at
step 0, which is the case the composition can express (ragged rows and ragged starts would cost it masks on top).  Alternating
within the run:
    mutual_clearance_kernel "all"     every output
    mutual_clearance_kernel "rows"    clearance and partner only: what autograd.mutual_clearance asks for
    mutual_clearance_vjp_kernel       dL/dsamples of sum(relu(2 - clearance))
    torch forward                     the composition, clearance and partner (torch.min over the neighbour axis)
    torch forward + backward          the same and .backward() of the same loss
The kernels (ids 35, 36) are timed by the library's own per-dispatch events; the composition is a dozen launches, timed by torch
events around it, so its figure includes its launches' gaps -- which is what its user pays.  Prints one JSON line per
configuration: medians in microseconds, the composition's peak temporary, the agreement of the two (clearance to 1e-12, partner
exactly, the gradient to 1e-12 of its largest entry), and the bytes the kernels must move at the least (every row read once,
every output written once) with the rate that makes.
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api  # noqa: E402

RADIUS = 2.0


def make_rows(G, N, Q, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(dtype=torch.float64, device="cuda")
    start = torch.rand((G * N, 1, 3), generator=gen, **kw) * 20.0
    steps = torch.randn((G * N, Q, 3), generator=gen, **kw) * 0.1
    rows = torch.zeros((G * N, Q, 4), **kw)
    # (not clamped into the box: paths pressed into one corner would coincide exactly, where the composition's sqrt has no
    # derivative and the step gives 0)
    rows[..., :3] = start + torch.cumsum(steps, dim=1)
    return rows


def torch_composition(rows, G, N):
    """(clearance [G N][Q], partner [G N][Q]) by the pairwise expression; differentiable in rows"""
    Q = rows.shape[1]
    x = rows[..., :3].reshape(G, N, Q, 3)
    d = x[:, :, None] - x[:, None, :]                         # [G][N][N][Q][3]
    c = d.pow(2).sum(-1).sqrt()                               # (sqrt(0) on the diagonal: masked below, before any gradient)
    eye = torch.eye(N, dtype=torch.bool, device=rows.device)[None, :, :, None]
    c = torch.where(eye, torch.full_like(c, float("inf")), c)
    best, j = c.min(dim=2)
    return best.reshape(G * N, Q), (j + (torch.arange(G, device=rows.device) * N)[:, None, None]).reshape(G * N, Q).to(torch.int32)


def torch_loss(rows, G, N):
    Q = rows.shape[1]
    x = rows[..., :3].reshape(G, N, Q, 3)
    d = x[:, :, None] - x[:, None, :]
    eye = torch.eye(N, dtype=torch.bool, device=rows.device)[None, :, :, None, None]
    d = torch.where(eye, torch.ones_like(d), d)               # (keeps sqrt'(0) = inf out of the backward pass)
    c = d.pow(2).sum(-1).sqrt()
    c = torch.where(eye[..., 0], torch.full_like(c, float("inf")), c)
    return torch.relu(RADIUS - c.min(dim=2)[0]).sum()


def measure(ctx, G, N, Q, reps):
    P = G * N
    rows = make_rows(G, N, Q, 1234)
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    n = torch.full((P,), Q, **i32)
    off = torch.arange(0, P + 1, N, **i32)
    c, q = torch.empty((P, Q), **f64), torch.empty((P, Q), **i32)
    mn, arg = torch.empty(P, **f64), torch.empty((P, 2), **i32)
    gs = torch.empty((P, Q, 4), **f64)
    plan.mutual_clearance(rows, n, off, clearance=c, partner=q)
    up = -(c < RADIUS).to(torch.float64)                      # dL/dclearance of sum(relu(RADIUS - clearance))
    out = OrderedDict((k, []) for k in ("fwd_all", "fwd_rows", "vjp", "torch_fwd", "torch_fwd_bwd"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    peak = 0
    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["fwd_all"] = timed(api.KERNEL_MUTUAL_CLEARANCE, lambda: plan.mutual_clearance(
            rows, n, off, clearance=c, partner=q, min_clearance=mn, argmin=arg))
        got["fwd_rows"] = timed(api.KERNEL_MUTUAL_CLEARANCE, lambda: plan.mutual_clearance(rows, n, off, clearance=c, partner=q))
        got["vjp"] = timed(api.KERNEL_MUTUAL_CLEARANCE_VJP, lambda: plan.mutual_clearance_vjp(rows, n, off, q, up, gs))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        ev[0].record()
        with torch.no_grad():
            tc, tq = torch_composition(rows, G, N)
        ev[1].record()
        leaf = rows.detach().requires_grad_(True)
        ev[2].record()
        torch_loss(leaf, G, N).backward()
        ev[3].record()
        torch.cuda.synchronize()
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        if r >= 2:   # (the first two rounds: code upload, the allocator's first blocks)
            out["torch_fwd"].append(ev[0].elapsed_time(ev[1]))
            out["torch_fwd_bwd"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    # the two routes agree
    gt = leaf.grad
    agree = OrderedDict(clearance_max_abs_diff=float((c - tc).abs().max()), partners_differ=int((q != tq).sum()),
                        gradient_max_abs_diff=float((gs - gt).abs().max()), gradient_max_abs=float(gt.abs().max()),
                        least_clearance=float(c.min()), rows_inside_the_hinge=int((c < RADIUS).sum()))
    assert bool(torch.all(torch.isfinite(c))) and agree["clearance_max_abs_diff"] <= 1e-12 and agree["partners_differ"] == 0, agree
    assert agree["gradient_max_abs_diff"] <= 1e-12 * agree["gradient_max_abs"] and not bool(gs[..., 3].any()), agree
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(config="%dx%dx%d" % (G, N, Q), paths=P, rows=P * Q, pairs_per_row=N - 1, reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res.update(agree)
    res["torch_peak_temporary_MB"] = round(peak / 1e6, 1)
    least = P * Q * (32 + 8 + 4)          # every row read once, clearance and partner written once
    res["fwd_rows_least_bytes_MB"] = round(least / 1e6, 2)
    res["fwd_rows_GBps_of_least_bytes"] = round(least / (med["fwd_rows"] * 1e-6) / 1e9, 1)
    res["fwd_rows_pair_distances_per_ns"] = round(P * Q * (N - 1) / (med["fwd_rows"] * 1e3), 2)
    res["torch_fwd_over_fwd_rows"] = round(med["torch_fwd"] / med["fwd_rows"], 1)
    res["torch_fwd_bwd_over_fwd_rows_plus_vjp"] = round(med["torch_fwd_bwd"] / (med["fwd_rows"] + med["vjp"]), 1)
    res["library"] = os.path.basename(api.LIB_PATH)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="64x16x512,8x128x512")
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        G, N, Q = (int(t) for t in cfg.split("x"))
        print(json.dumps(measure(ctx, G, N, Q, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

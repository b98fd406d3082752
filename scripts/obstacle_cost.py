#!/usr/bin/env python3
"""What the clearance from static obstacles and its backward pass cost: obstacle_clearance_kernel
(mrs_tg_plan_obstacle_clearance, one workgroup per path, one lane per row, the obstacles of the path's set the inner loop, read
as wavefront-uniform data) and obstacle_clearance_vjp_kernel (mrs_tg_plan_obstacle_clearance_vjp, one lane per row) against the
torch composition that was the only route before the step existed -- rows [N][Q][3] against obstacles [M][4] by broadcasting:
differences [N][Q][M][3] -> norm -> minus the radius -> min and argmin over the obstacles, and its autograd backward -- on the GPU.

    python scripts/obstacle_cost.py [--reps 20] [--configs shared:64,shared:1024,shared:4096,perpath:64] [--paths 1024] [--rows 512]

shared:M is one set of M obstacles that every path sees, perpath:M one set of M obstacles per path.  The rows are random walks
of 0.1 m steps from starts in a 20 m box and the obstacles are drawn in the same box, every other one a point, the rest spheres
of 0.1 .. 0.5 m, all on the device from a seed; every path has all its rows, which is the case the composition can express
without a mask.  Alternating within the run:
    obstacle_clearance_kernel "all"     every output
    obstacle_clearance_kernel "rows"    clearance and nearest only: what autograd.obstacle_clearance asks for
    obstacle_clearance_vjp_kernel       dL/dsamples of sum(relu(1 - clearance))
    torch forward                       the composition, clearance and nearest (torch.min over the obstacle axis)
    torch forward + backward            the same and .backward() of the same loss
The kernels (ids 37, 38) are timed by the library's own per-dispatch events; the composition is a dozen launches, timed by torch
events around it, so its figure includes its launches' gaps -- which is what its user pays.  WHERE THE COMPOSITION'S TEMPORARIES
WOULD NOT FIT (an [N][Q][M] double array is 17 GB at 1024 x 512 x 4096, and autograd keeps a dozen of that size) IT RUNS IN
CHUNKS OF PATHS, one after the other inside the timed window, and the line says so: torch_chunk_paths.  Prints one JSON line
per configuration: medians in microseconds, the composition's peak temporary, the agreement of the two (clearance to 1e-12,
nearest exactly, the gradient to 1e-12 of its largest entry), the pairs per nanosecond and the share of the device's FP64
instruction issue rate the forward reaches AT THE LEAST: FP64_PER_PAIR double-precision vector instructions per (row, obstacle)
pair on the route that spares the square root (obsq::cannot_win; the groups of four obstacles that take the root issue
FP64_PER_PAIR_WITH_ROOT, and how many do is not counted), read from the kernel's disassembly, against one such instruction per
SIMD every four cycles (16 lanes per cycle, half the FP32 rate) on 256 CUs x 4 SIMDs at 2.4 GHz.
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

RADIUS = 1.0
# vector instructions of obstacle_clearance_kernel's unrolled loop per pair, from its disassembly: the
# route that spares the root is 15, all of them v_*_f64; the root adds 24, 16 of them v_*_f64
FP64_PER_PAIR, FP64_PER_PAIR_WITH_ROOT = 15, 31
VALU_PER_PAIR, VALU_PER_PAIR_WITH_ROOT = 15, 39
FP64_LANES_PER_S = 256 * 4 * 16 * 2.4e9
TORCH_TEMPORARY_BUDGET = 24e9   # bytes the composition's live [chunk][Q][M] temporaries may take (a dozen of them, forward + backward)


def make_rows(P, Q, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(dtype=torch.float64, device="cuda")
    start = torch.rand((P, 1, 3), generator=gen, **kw) * 20.0
    steps = torch.randn((P, Q, 3), generator=gen, **kw) * 0.1
    rows = torch.zeros((P, Q, 4), **kw)
    rows[..., :3] = start + torch.cumsum(steps, dim=1)
    return rows


def make_obstacles(M, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    kw = dict(dtype=torch.float64, device="cuda")
    ob = torch.zeros((M, 4), **kw)
    ob[:, :3] = torch.rand((M, 3), generator=gen, **kw) * 20.0
    ob[1::2, 3] = 0.1 + 0.4 * torch.rand((ob[1::2].shape[0],), generator=gen, **kw)
    return ob


def torch_composition(rows, ob):
    """(clearance [n][Q], nearest [n][Q]) of rows [n][Q][4] against ob [M][4] (every path sees them) or [n][M][4] (a set per
    path) by the broadcast expression; differentiable in rows.  The index counts within the set."""
    o = ob[None, None] if ob.dim() == 2 else ob[:, None]           # [1 or n][1][M][4]
    d = rows[:, :, None, :3] - o[..., :3]                         # [n][Q][M][3]
    c = d.pow(2).sum(-1).sqrt() - o[..., 3]
    return c.min(dim=2)


def chunks(P, Q, M):
    per_path = Q * M * 8 * 12
    n = int(max(1, min(P, TORCH_TEMPORARY_BUDGET // per_path)))
    return 1 << (n.bit_length() - 1)          # a power of two, so that it divides the usual path counts


def measure(ctx, kind, M, P, Q, reps):
    rows = make_rows(P, Q, 1234)
    per_path = kind == "perpath"
    S = P if per_path else 1
    ob = make_obstacles(S * M, 4321)
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    n = torch.full((P,), Q, **i32)
    off = torch.arange(0, S * M + 1, M, **i32)
    ps = torch.arange(P, **i32) if per_path else None
    c, q = torch.empty((P, Q), **f64), torch.empty((P, Q), **i32)
    mn, arg = torch.empty(P, **f64), torch.empty((P, 2), **i32)
    gs = torch.empty((P, Q, 4), **f64)
    plan.obstacle_clearance(rows, n, ob, off, path_set=ps, clearance=c, nearest=q)
    up = -(c < RADIUS).to(torch.float64)                      # dL/dclearance of sum(relu(RADIUS - clearance))
    out = OrderedDict((k, []) for k in ("fwd_all", "fwd_rows", "vjp", "torch_fwd", "torch_fwd_bwd"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    step = chunks(P, Q, M)
    tc, tq = torch.empty((P, Q), **f64), torch.empty((P, Q), dtype=torch.int64, device="cuda")
    gt = torch.empty((P, Q, 4), **f64)

    def ob_of(a, b):
        return ob.view(P, M, 4)[a:b] if per_path else ob

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    peak = 0
    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["fwd_all"] = timed(api.KERNEL_OBSTACLE_CLEARANCE, lambda: plan.obstacle_clearance(
            rows, n, ob, off, path_set=ps, clearance=c, nearest=q, min_clearance=mn, argmin=arg))
        got["fwd_rows"] = timed(api.KERNEL_OBSTACLE_CLEARANCE, lambda: plan.obstacle_clearance(
            rows, n, ob, off, path_set=ps, clearance=c, nearest=q))
        got["vjp"] = timed(api.KERNEL_OBSTACLE_CLEARANCE_VJP, lambda: plan.obstacle_clearance_vjp(
            rows, n, ob, off, q, up, gs, path_set=ps))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        ev[0].record()
        with torch.no_grad():
            for a in range(0, P, step):
                tc[a:a + step], tq[a:a + step] = torch_composition(rows[a:a + step], ob_of(a, a + step))
        ev[1].record()
        ev[2].record()
        for a in range(0, P, step):
            leaf = rows[a:a + step].detach().requires_grad_(True)
            torch.relu(RADIUS - torch_composition(leaf, ob_of(a, a + step))[0]).sum().backward()
            gt[a:a + step] = leaf.grad
        ev[3].record()
        torch.cuda.synchronize()
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        if r >= 2:   # (the first two rounds: code upload, the allocator's first blocks)
            out["torch_fwd"].append(ev[0].elapsed_time(ev[1]))
            out["torch_fwd_bwd"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    # the two routes agree
    tq_whole = tq + (torch.arange(P, device="cuda") * M)[:, None] if per_path else tq
    agree = OrderedDict(clearance_max_abs_diff=float((c - tc).abs().max()), nearest_differ=int((q != tq_whole).sum()),
                        gradient_max_abs_diff=float((gs - gt).abs().max()), gradient_max_abs=float(gt.abs().max()),
                        least_clearance=float(c.min()), rows_inside_the_hinge=int((c < RADIUS).sum()))
    assert bool(torch.all(torch.isfinite(c))) and agree["clearance_max_abs_diff"] <= 1e-12 and agree["nearest_differ"] == 0, agree
    assert agree["gradient_max_abs_diff"] <= 1e-12 * agree["gradient_max_abs"] and not bool(gs[..., 3].any()), agree
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(config="%s:%d" % (kind, M), paths=P, rows=P * Q, obstacles=S * M, pairs_per_row=M, reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res.update(agree)
    res["torch_chunk_paths"] = step
    res["torch_runs_in_chunks"] = step < P
    res["torch_peak_temporary_MB"] = round(peak / 1e6, 1)
    pairs = P * Q * M
    res["fwd_rows_pairs_per_ns"] = round(pairs / (med["fwd_rows"] * 1e3), 2)
    res["fwd_rows_least_share_of_fp64_issue_rate"] = round(pairs * FP64_PER_PAIR / (med["fwd_rows"] * 1e-6) / FP64_LANES_PER_S, 3)
    res["fp64_instructions_per_pair"] = [FP64_PER_PAIR, FP64_PER_PAIR_WITH_ROOT]
    res["vector_instructions_per_pair"] = [VALU_PER_PAIR, VALU_PER_PAIR_WITH_ROOT]
    res["torch_fwd_over_fwd_rows"] = round(med["torch_fwd"] / med["fwd_rows"], 1)
    res["torch_fwd_bwd_over_fwd_rows_plus_vjp"] = round(med["torch_fwd_bwd"] / (med["fwd_rows"] + med["vjp"]), 1)
    res["library"] = os.path.basename(api.LIB_PATH)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="shared:64,shared:1024,shared:4096,perpath:64")
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=512)
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        kind, M = cfg.split(":")
        assert kind in ("shared", "perpath"), cfg
        print(json.dumps(measure(ctx, kind, int(M), a.paths, a.rows, a.reps)), flush=True)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

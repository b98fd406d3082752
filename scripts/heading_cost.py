#!/usr/bin/env python3
"""What the heading along the direction of travel and its backward pass cost, and how accurate the heading is:
travel_heading_kernel (mrs_tg_plan_travel_heading, one wavefront per path, sources by one ballot per chunk) in place and out of
place and travel_heading_vjp_kernel (mrs_tg_plan_travel_heading_vjp), beside path_deviation_kernel at the same shape -- it reads
the same rows with the same walk -- and beside the host loop of mrs_tg_policy_host.hpp (getTrajectoryReference :1578-1603)
restated in numpy, vectorised over the paths and serial over the rows -- on the GPU.

    python scripts/heading_cost.py [--reps 20] [--configs 1024x200,10240x200] [--accuracy 1] > profiles/heading_cost.txt

Rows are built directly: positions are cumulative sums of steps in drawn directions, one step in ten shorter than 0.05 m.  The
kernels are timed by the library's own per-dispatch events (kernel ids 23, 24 and 8); the numpy loop by a host clock.  Bytes per
row: 32 B read, and 8 B (in place: the heading) or 32 B (out of place: the row) written; the backward pass reads 64 B (the row and
its upstream) and writes 32 B.  Prints one JSON line per configuration: medians in microseconds, achieved bytes/s, the ratios.

--accuracy 1 adds the heading's accuracy: the device's atan2 against the C library's (math.atan2) and against np.arctan2 on
bit-identical (dx, dy) -- over every row of the larger batch in two draws (at least 4e6 rows), and over 1e5 ratios dy/dx,
logarithmic from 1e-300 to 1e300, in all four quadrants (paths of two rows from the origin: the step is the operand pair
itself).  tests/heading_util.py takes its bound from that line."""
import argparse
import json
import math
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api  # noqa: E402

MIN_STEP = 0.05


def draw_rows(n_paths, n_rows, seed):
    rng = np.random.default_rng(seed)
    length = np.where(rng.random((n_paths, n_rows - 1)) < 0.1, rng.uniform(0.0, 0.049, (n_paths, n_rows - 1)),
                      rng.uniform(0.051, 0.6, (n_paths, n_rows - 1)))
    angle = rng.uniform(-math.pi, math.pi, (n_paths, n_rows - 1))
    rows = np.zeros((n_paths, n_rows, 4))
    rows[:, 0, :2] = rng.uniform(-5.0, 5.0, (n_paths, 2))
    rows[:, 1:, 0] = rows[:, :1, 0] + np.cumsum(length * np.cos(angle), axis=1)
    rows[:, 1:, 1] = rows[:, :1, 1] + np.cumsum(length * np.sin(angle), axis=1)
    rows[:, :, 2] = rng.uniform(1.0, 4.0, (n_paths, n_rows))
    rows[:, :, 3] = rng.uniform(-3.0, 3.0, (n_paths, n_rows))
    return rows


def host_loop(rows):
    """mrs_tg_policy_host.hpp:700-709 for every path at once: serial over the rows, as the loop is"""
    out = rows.copy()
    for it in range(rows.shape[1] - 1):
        dy, dx = rows[:, it + 1, 1] - rows[:, it, 1], rows[:, it + 1, 0] - rows[:, it, 0]
        own = np.arctan2(dy, dx)
        if it > 0:
            own = np.where(np.hypot(dy, dx) < MIN_STEP, out[:, it - 1, 3], own)
        out[:, it, 3] = own
    return out


def heading_errors(rows, got, source):
    """worst |device heading - atan2 of the same (dx, dy)| over the rows 0 .. n-2, against math.atan2 and against np.arctan2"""
    d = rows[:, 1:, :2] - rows[:, :-1, :2]
    src = source[:, :-1].astype(np.int64)
    dx, dy = np.take_along_axis(d[:, :, 0], src, axis=1).ravel(), np.take_along_axis(d[:, :, 1], src, axis=1).ravel()
    h = got[:, :-1, 3].ravel()
    libm = np.fromiter(map(math.atan2, dy.tolist(), dx.tolist()), dtype=np.float64, count=h.size)
    return h.size, float(np.max(np.abs(h - libm))), float(np.max(np.abs(h - np.arctan2(dy, dx))))


def run_heading(ctx, rows):
    """-> (rows out, source) of one out-of-place call"""
    P, n_rows = rows.shape[:2]
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    s = torch.from_numpy(rows).cuda()
    n = torch.full((P,), n_rows, dtype=torch.int32, device="cuda")
    out = torch.empty_like(s)
    source = torch.empty((P, n_rows), dtype=torch.int32, device="cuda")
    plan.travel_heading(s, n, samples_out=out, source=source)
    torch.cuda.synchronize()
    plan.close()
    return out.cpu().numpy(), source.cpu().numpy()


def accuracy(ctx, n_paths, n_rows):
    res = OrderedDict(rows=0, worst_vs_libm=0.0, worst_vs_numpy=0.0)
    for seed in (1, 2):
        rows = draw_rows(n_paths, n_rows, seed)
        got, source = run_heading(ctx, rows)
        k, a, b = heading_errors(rows, got, source)
        res["rows"] += k
        res["worst_vs_libm"], res["worst_vs_numpy"] = max(res["worst_vs_libm"], a), max(res["worst_vs_numpy"], b)
    ratio = np.logspace(-300.0, 300.0, 100000)
    pairs = np.concatenate([np.stack([sx * np.ones_like(ratio), sy * ratio], axis=1) for sx in (1.0, -1.0) for sy in (1.0, -1.0)])
    rows = np.zeros((pairs.shape[0], 2, 4))
    rows[:, 1, :2] = pairs
    got, source = run_heading(ctx, rows)
    k, a, b = heading_errors(rows, got, source)
    res.update(sweep_pairs=k, sweep_worst_vs_libm=a, sweep_worst_vs_numpy=b)
    res["worst"] = max(res["worst_vs_libm"], res["worst_vs_numpy"], a, b)
    res["worst_in_units_of_2^-53"] = res["worst"] * 2.0 ** 53
    return res


def measure(ctx, n_paths, n_rows, reps, n_seg=10):
    rows = draw_rows(n_paths, n_rows, 0)
    P = n_paths
    f64, i32 = dict(dtype=torch.float64, device="cuda"), dict(dtype=torch.int32, device="cuda")
    s = torch.from_numpy(rows).cuda()
    n = torch.full((P,), n_rows, **i32)
    out, work = torch.empty_like(s), s.clone()
    source = torch.empty((P, n_rows), **i32)
    up = torch.randn((P, n_rows, 4), generator=torch.Generator(device="cuda").manual_seed(0), **f64)
    gs = torch.empty_like(s)
    # the deviation step on the same rows: a plan of n_seg segments per path, waypoints picked from the rows themselves
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32) * n_seg)
    pick = np.linspace(0, n_rows - 1, n_seg + 1).astype(np.int64)
    wp = torch.from_numpy(np.ascontiguousarray(rows[:, pick, :].reshape(-1, 4))).cuda()
    dev, mx = torch.empty((P, n_rows), **f64), torch.empty(P, **f64)
    t = OrderedDict((k, []) for k in ("in_place", "out_of_place", "out_of_place_with_source", "vjp", "deviation"))

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["in_place"] = timed(api.KERNEL_TRAVEL_HEADING, lambda: plan.travel_heading(work, n))
        got["out_of_place"] = timed(api.KERNEL_TRAVEL_HEADING, lambda: plan.travel_heading(s, n, samples_out=out))
        got["out_of_place_with_source"] = timed(api.KERNEL_TRAVEL_HEADING,
                                                lambda: plan.travel_heading(s, n, samples_out=out, source=source))
        got["vjp"] = timed(api.KERNEL_TRAVEL_HEADING_VJP, lambda: plan.travel_heading_vjp(s, n, up, gs))
        got["deviation"] = timed(api.KERNEL_DEVIATION, lambda: plan.path_deviation(s, n, wp, deviation=dev, max_deviation=mx))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            for k, v in got.items():
                t[k] += v
    plan.close()
    assert torch.equal(work[:, :, :3], s[:, :, :3]) and torch.equal(work.view(torch.int64), out.view(torch.int64))
    t0 = time.perf_counter()
    host = host_loop(rows)
    host_us = (time.perf_counter() - t0) * 1e6
    src = source.cpu().numpy()
    med = {k: float(np.median(v)) * 1e3 for k, v in t.items()}
    n_all = P * n_rows
    res = OrderedDict(config="%dx%d" % (P, n_rows), rows=n_all, reps=reps,
                      carried_rows=int(np.sum(src[:, :-1] != np.arange(n_rows - 1)[None, :])),
                      worst_vs_numpy_host_loop=float(np.max(np.abs(out.cpu().numpy()[:, :-1, 3] - host[:, :-1, 3]))))
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["numpy_host_loop_us"] = round(host_us, 1)
    res["in_place_GBps"] = round(n_all * 40 / med["in_place"] / 1e3, 1)
    res["out_of_place_GBps"] = round(n_all * 64 / med["out_of_place"] / 1e3, 1)
    res["vjp_GBps"] = round(n_all * 96 / med["vjp"] / 1e3, 1)
    res["out_of_place_over_in_place"] = round(med["out_of_place"] / med["in_place"], 3)
    res["in_place_over_deviation"] = round(med["in_place"] / med["deviation"], 3)
    res["vjp_over_out_of_place"] = round(med["vjp"] / med["out_of_place"], 3)
    res["numpy_host_loop_over_in_place"] = round(host_us / med["in_place"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="1024x200,10240x200")
    ap.add_argument("--accuracy", type=int, default=0)
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    shapes = [tuple(int(v) for v in cfg.split("x")) for cfg in a.configs.split(",")]
    for P, n_rows in shapes:
        print(json.dumps(measure(ctx, P, n_rows, a.reps)), flush=True)
    if a.accuracy:
        P, n_rows = max(shapes)
        print(json.dumps(dict(accuracy=accuracy(ctx, P, n_rows))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

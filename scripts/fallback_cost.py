#!/usr/bin/env python3
"""What the fallback sampler as a plan step, its backward pass and the heading unwrap cost: fallback_sample_kernel
(mrs_tg_plan_fallback_sample), fallback_sample_vjp_kernel (mrs_tg_plan_fallback_sample_vjp) and unwrap_headings_kernel
(mrs_tg_plan_unwrap_headings) on the GPU, beside two yardsticks measured in the same run: the polynomial sampler
(mrs_tg_plan_sample) on a solved batch of the same shape, per row written, and path_deviation_vjp_kernel on the fallback's own
rows (the same row count), which sums its waypoint rows through an LDS tile the way the fallback's backward pass does.

    python scripts/fallback_cost.py [--reps 30] [--configs 10240x10,65536x10] [--dt 0.2]

Random paths at the bench's limits, the clock is the Baca estimate of the unwrapped waypoints (mrs_tg_plan_unwrap_headings, then
mrs_tg_plan_estimate_times_baca).  The three new kernels and the deviation's backward pass are timed by the library's own
per-dispatch events (kernel ids 17, 18, 19 and 9); the polynomial sampler has no event id and is timed by torch events around
the call (launch included), and so, beside its event time, is the fallback's forward: that pair is the like-for-like one.  The
compulsory traffic of the forward: 32 B written per row, about 40 B read per segment (a waypoint row, a time, a stop flag); of
the backward pass: 32 B read per row, 32 B written per vertex.  Prints one JSON line per configuration: medians in
microseconds, rows, nanoseconds per row, achieved GB/s and the fraction of the HBM peak given with --peak-gbps."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402


def measure(ctx, n_paths, n_seg, reps, dt, peak_gbps):
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    nS, P = batch.n_segments, batch.n_paths
    nV = nS + P
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    # the polynomial yardstick: a solved batch of the same shape and its sample counts
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    n_poly = torch.zeros(P, **i32)
    plan.sample_states_vjp(db.coeffs, db.seg_times, dt, 1 << 20, None, n_samples=n_poly)
    # the fallback's clock and counts
    wp = db.waypoints
    unwrapped = torch.empty_like(wp)
    t_baca = torch.empty(nS, **f64)
    plan.unwrap_headings(wp, unwrapped)
    plan.estimate_times_baca(unwrapped, db.limits, t_baca)
    gen = torch.Generator(device="cuda").manual_seed(0)
    stop = (torch.rand(nV, device="cuda", generator=gen) < 0.1).to(torch.uint8)
    n_fb = torch.zeros(P, **i32)
    torch.cuda.synchronize()
    # the capacity that holds every path: the row rule on the host (the kernel's counts are checked against it below)
    t = t_baca.cpu().numpy()
    nd = np.where(t > 0.1, np.ceil(t / dt), 0.0)
    so = np.asarray(batch.seg_offsets)
    last = np.zeros(nS, dtype=bool)
    last[so[1:] - 1] = True
    first_vertex = np.zeros(nV, dtype=bool)
    first_vertex[so[:-1] + np.arange(P)] = True
    seg_vertex = np.arange(nS) + np.searchsorted(so, np.arange(nS), side="right") - 1
    stop_h = stop.cpu().numpy().astype(bool)
    rows_seg = nd + (last & (nd > 0)) + np.where((nd > 0) & stop_h[seg_vertex] & ~first_vertex[seg_vertex], round(2.0 / dt), 0)
    per_path = np.add.reduceat(rows_seg, so[:-1]).astype(np.int64)
    cap_fb, cap_poly = int(per_path.max()), int(n_poly.max().item())
    s_fb, s_poly = torch.empty((P, cap_fb, 4), **f64), torch.zeros((P, cap_poly, 4), **f64)
    first = torch.empty(nS, **i32)
    G = torch.randn((P, cap_fb, 4), generator=gen, **f64)
    Gd = torch.randn((P, cap_fb), generator=gen, **f64)
    gw, gs = torch.empty((nV, 4), **f64), torch.empty((P, cap_fb, 4), **f64)
    out = OrderedDict((k, []) for k in ("unwrap", "fallback_forward", "fallback_forward_no_first_row", "fallback_vjp",
                                        "deviation_vjp_same_rows", "fallback_forward_torch_events", "poly_sample_torch_events"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ev[0].record()
        plan.sample(db.coeffs, db.seg_times, dt, cap_poly, n_poly, s_poly)
        ev[1].record()
        ev[2].record()
        plan.fallback_sample(wp, t_baca, dt, cap_fb, n_fb, s_fb, stop_at=stop)
        ev[3].record()
        ctx.set_profiling(True)
        got = OrderedDict()
        got["unwrap"] = timed(api.KERNEL_UNWRAP_HEADINGS, lambda: plan.unwrap_headings(wp, unwrapped))
        got["fallback_forward"] = timed(api.KERNEL_FALLBACK_SAMPLE, lambda: plan.fallback_sample(
            wp, t_baca, dt, cap_fb, n_fb, s_fb, stop_at=stop, seg_first_row=first))
        got["fallback_forward_no_first_row"] = timed(api.KERNEL_FALLBACK_SAMPLE, lambda: plan.fallback_sample(
            wp, t_baca, dt, cap_fb, n_fb, s_fb, stop_at=stop))
        got["fallback_vjp"] = timed(api.KERNEL_FALLBACK_SAMPLE_VJP, lambda: plan.fallback_sample_vjp(
            t_baca, dt, cap_fb, G, gw, stop_at=stop))
        got["deviation_vjp_same_rows"] = timed(api.KERNEL_DEVIATION_VJP, lambda: plan.path_deviation_vjp(
            s_fb, n_fb, wp, Gd, grad_samples=gs, grad_waypoints=gw))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["poly_sample_torch_events"].append(ev[0].elapsed_time(ev[1]))
            out["fallback_forward_torch_events"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    rows_fb = int(n_fb.to(torch.int64).sum().item())
    assert rows_fb == int(per_path.sum()), (rows_fb, int(per_path.sum()))      # the host's sizing is the kernel's count
    rows_poly = int(torch.minimum(n_poly, torch.tensor(cap_poly, **i32)).to(torch.int64).sum().item())
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    fwd_bytes = 32 * rows_fb + 40 * nS + 32 * P + 4 * P
    vjp_bytes = 32 * rows_fb + 32 * nV + 9 * nS
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, reps=reps, dt=dt, rows_fallback=rows_fb, rows_poly=rows_poly,
                      capacity_fallback=cap_fb, capacity_poly=cap_poly)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["fallback_forward_ns_per_row"] = round(med["fallback_forward"] * 1e3 / rows_fb, 4)
    res["fallback_forward_torch_events_ns_per_row"] = round(med["fallback_forward_torch_events"] * 1e3 / rows_fb, 4)
    res["poly_sample_torch_events_ns_per_row"] = round(med["poly_sample_torch_events"] * 1e3 / rows_poly, 4)
    res["fallback_over_poly_per_row"] = round(res["fallback_forward_torch_events_ns_per_row"] /
                                              res["poly_sample_torch_events_ns_per_row"], 2)
    res["fallback_forward_bytes"], res["fallback_vjp_bytes"] = fwd_bytes, vjp_bytes
    res["fallback_forward_GBps"] = round(fwd_bytes / med["fallback_forward"] * 1e-3, 1)
    res["fallback_forward_fraction_of_peak"] = round(res["fallback_forward_GBps"] / peak_gbps, 3)
    res["fallback_vjp_GBps"] = round(vjp_bytes / med["fallback_vjp"] * 1e-3, 1)
    res["fallback_vjp_ns_per_row"] = round(med["fallback_vjp"] * 1e3 / rows_fb, 4)
    res["deviation_vjp_ns_per_row"] = round(med["deviation_vjp_same_rows"] * 1e3 / rows_fb, 4)
    res["fallback_vjp_over_deviation_vjp"] = round(med["fallback_vjp"] / med["deviation_vjp_same_rows"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--configs", default="10240x10,65536x10")
    ap.add_argument("--dt", type=float, default=0.2)
    ap.add_argument("--peak-gbps", type=float, default=8000.0, help="HBM peak of the device (MI355X: 8 TB/s)")
    a = ap.parse_args()
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for cfg in a.configs.split(","):
        n, s = cfg.split("x")
        print(json.dumps(measure(ctx, int(n), int(s), a.reps, a.dt, a.peak_gbps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

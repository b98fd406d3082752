#!/usr/bin/env python3
"""What the waypoint passage and its backward pass cost: waypoint_passage_kernel (mrs_tg_plan_waypoint_passage, one wavefront
per path, the waypoint cursor by ballots) and waypoint_passage_vjp_kernel (mrs_tg_plan_waypoint_passage_vjp) against
path_deviation_kernel with every output on the same samples, against sample_kernel<0> (mrs_tg_plan_sample), which produced
them, and against the host route -- the samples copied down and mrs_tg_waypoint_trajectory_idxs called path by path -- on the
GPU.

    python scripts/passage_cost.py [--reps 20] [--dt 0.2] [--configs 1024x10,4096x10,10240x10]
    python scripts/passage_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                         rocprofv3 --kernel-trace --stats run of the line above; a
                                                         kernel trace alone -- counters, if wanted, in a run of their own)

Per configuration the batch's times come from the library's estimator and its coefficients from the default fixed-times
solve; the samples are mrs_tg_plan_sample's at dt; the waypoints asked about are the plan's vertices.  Alternating within the
run: sample_kernel<0>, path_deviation_kernel (every output), waypoint_passage_kernel (every output),
waypoint_passage_vjp_kernel (both gradients, both upstreams), then the host route (wall clock: device-to-host copy of samples
and counts, then one mrs_tg_waypoint_trajectory_idxs per path through ctypes, the waypoint structs prepared beforehand).  The
timed families (kernel ids 8, 12, 13) are timed by the library's own per-dispatch events, sample_kernel<0> by torch events
around the call (launch included) -- the rocprofv3 summary is the like-for-like kernel comparison.  The script asserts that the
device's indices and counts are the host's.  Prints one JSON line per configuration: medians in microseconds, the ratios, and
the ballot rounds that explain the forward (per chunk of 64 steps that is run: the hits in it, plus one round that finds none
unless the chunk ends on a hit or on the last waypoint)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402
from scripts.deviation_cost import _trace_rows  # noqa: E402

KERNELS = ("sample_kernel", "path_deviation_kernel", "waypoint_passage")


def rounds_of(index, count, n, W):
    """ballot rounds per chunk of one path, as resolve_hits runs them: the chunks run while the cursor is short of W"""
    out, c = [], 0
    for k0 in range(0, max(n - 1, 0), 64):
        if c >= W:
            break
        last_open = min(k0 + 63, n - 2)
        rounds = 0
        while c < W:
            rounds += 1
            if c < count and index[c] <= last_open:   # a hit: the lanes up to it close
                c += 1
                if index[c - 1] == last_open:
                    break
            else:
                break
        out.append(rounds)
    return out


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
    nV = nS + P
    n_dev = torch.zeros(P, dtype=torch.int32, device="cuda")
    plan.sample_states_vjp(db.coeffs, db.seg_times, dt, 1 << 20, None, n_samples=n_dev)
    torch.cuda.synchronize()
    cap = int(n_dev.max().item())
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    samples = torch.zeros((P, cap, 4), **f64)
    dev, cur = torch.empty((P, cap), **f64), torch.empty((P, cap), **i32)
    mx, arg, seg = torch.empty(P, **f64), torch.empty(P, **i32), torch.empty(nS, **f64)
    index, count, miss, frac = torch.empty(nV, **i32), torch.empty(P, **i32), torch.empty(nV, **f64), torch.empty(nV, **f64)
    gen = torch.Generator(device="cuda").manual_seed(0)
    Gm, Gt = torch.randn(nV, generator=gen, **f64), torch.randn(nV, generator=gen, **f64)
    gs, gw = torch.empty((P, cap, 4), **f64), torch.empty((nV, 4), **f64)
    # the host route's inputs that a service holds already: the waypoints as mrs_tg_waypoint structs, per path
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    structs, _ = api._waypoint_array([batch.waypoints[so[p] + p:so[p + 1] + p + 1] for p in range(P)])
    wbase, wsize = structs.ctypes.data, structs.dtype.itemsize
    # (plain addresses: the loop below is the host's own work, not the wrapper's conversions)
    host_fn = C.cast(api.load_library().mrs_tg_waypoint_trajectory_idxs,
                     C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p))
    idx_host = np.full(nV, -1, dtype=np.int32)
    cnt_host = np.zeros(P, dtype=np.int32)
    out = OrderedDict((k, []) for k in ("sample", "dev_all", "passage", "passage_vjp", "host_copy", "host_scan"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ev[0].record()
        plan.sample(db.coeffs, db.seg_times, dt, cap, n_dev, samples)
        ev[1].record()
        ctx.set_profiling(True)
        got = OrderedDict()
        got["dev_all"] = timed(api.KERNEL_DEVIATION, lambda: plan.path_deviation(
            samples, n_dev, db.waypoints, first_segment=True, status=db.status, deviation=dev, cursor=cur, max_deviation=mx,
            argmax=arg, segment_max=seg))
        got["passage"] = timed(api.KERNEL_PASSAGE, lambda: plan.waypoint_passage(
            samples, n_dev, db.waypoints, status=db.status, index=index, count=count, miss=miss, fraction=frac))
        got["passage_vjp"] = timed(api.KERNEL_PASSAGE_VJP, lambda: plan.waypoint_passage_vjp(
            samples, n_dev, db.waypoints, grad_miss=Gm, grad_fraction=Gt, status=db.status, grad_samples=gs, grad_waypoints=gw))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smp = samples.cpu().numpy()
        n = n_dev.cpu().numpy()
        t1 = time.perf_counter()
        sbase, srow = smp.ctypes.data, smp.strides[0]
        for p in range(P):
            v0 = int(so[p]) + p
            cnt_host[p] = host_fn(sbase + p * srow, int(n[p]), wbase + v0 * wsize, int(so[p + 1] - so[p]) + 1,
                                  idx_host.ctypes.data + 4 * v0)
        t2 = time.perf_counter()
        if r >= 2:   # (the first two rounds: code upload)
            out["sample"].append(ev[0].elapsed_time(ev[1]))
            out["host_copy"].append((t1 - t0) * 1e3)
            out["host_scan"].append((t2 - t1) * 1e3)
            for k, v in got.items():
                out[k] += v
    # the device's indices are the host's
    idx, cnt = index.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(cnt, cnt_host)
    rounds = []
    for p in range(P):
        v0, W = int(so[p]) + p, int(so[p + 1] - so[p]) + 1
        k = int(cnt[p])
        assert np.array_equal(idx[v0:v0 + k], idx_host[v0:v0 + k]) and np.all(idx[v0 + k:v0 + W] == -1), p
        rounds += rounds_of(idx[v0:v0 + W], k, int(n[p]), W)
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), waypoints=nV, reached=int(cnt.sum()), samples=int(n.sum()), per_path=cap,
                      dt=dt, reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["host_route_us"] = round(med["host_copy"] + med["host_scan"], 2)
    res["chunks_run"] = len(rounds)
    res["chunks_of_the_samples"] = int(np.sum((np.maximum(n - 1, 0) + 63) // 64))
    res["ballot_rounds_per_chunk"] = round(float(np.mean(rounds)), 2)
    res["most_rounds_in_a_chunk"] = int(np.max(rounds))
    res["passage_over_dev_all"] = round(med["passage"] / med["dev_all"], 3)
    res["host_route_over_passage"] = round((med["host_copy"] + med["host_scan"]) / med["passage"], 1)
    res["passage_over_sample_kernel0_event"] = round(med["passage"] / med["sample"], 2)
    res["passage_vjp_over_sample_kernel0_event"] = round(med["passage_vjp"] / med["sample"], 2)
    return res


def summarize(path):
    """kernel trace -> per kernel name (in order of first appearance) and grid: dispatches, median / min / max us, registers"""
    rows = sorted(_trace_rows(path), key=lambda r: int(r["Start_Timestamp"]))
    groups = OrderedDict()
    for r in rows:
        name = r.get("Kernel_Name", "").replace("void ", "").replace("mrs_tg::", "").split("(")[0]
        if not any(s in name for s in KERNELS):
            continue
        grid, wg = r.get("Grid_Size_X", r.get("Grid_Size", "")), r.get("Workgroup_Size_X", r.get("Workgroup_Size", ""))
        g = groups.setdefault((name, grid, wg), dict(t=[], vgpr=r.get("VGPR_Count", r.get("Arch_VGPR_Count", "")),
                                                     agpr=r.get("Accum_VGPR_Count", ""), sgpr=r.get("SGPR_Count", ""),
                                                     scratch=r.get("Scratch_Size", r.get("Private_Segment_Size", ""))))
        g["t"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# kernel                         grid_x   wg    n  median_us     min_us     max_us  vgpr agpr sgpr scratch")
    for (name, grid, wg), g in groups.items():
        t = np.array(g["t"])
        print("  %-28s %8s %4s %4d %10.2f %10.2f %10.2f  %4s %4s %4s %s" % (name[:28], grid, wg, t.size, np.median(t), t.min(), t.max(),
                                                                          g["vgpr"], g["agpr"], g["sgpr"], g["scratch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=0.2)
    ap.add_argument("--configs", default="1024x10,4096x10,10240x10")
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

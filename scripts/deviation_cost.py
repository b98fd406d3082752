#!/usr/bin/env python3
"""What the deviation from the waypoint path and its backward pass cost: path_deviation_kernel (mrs_tg_plan_path_deviation,
one wavefront per path, cursors by ballots) and path_deviation_vjp_kernel (mrs_tg_plan_path_deviation_vjp) against
policy_validate_kernel (one lane per path, the scan as a loop; the kernel mrs_tg_optimize_paths runs) on the same samples, and
against sample_kernel<0> (mrs_tg_plan_sample), which produced them -- on the GPU.

    python scripts/deviation_cost.py [--reps 20] [--dt 0.2] [--configs 1024x10,4096x10,10240x10]
    python scripts/deviation_cost.py --summarize TRACE    (TRACE: the kernel_trace.csv or the results .db of a
                                                           rocprofv3 --kernel-trace --stats run of the line above; a
                                                           kernel trace alone -- counters, if wanted, in a run of their own)

Per configuration the batch's times come from the library's estimator and its coefficients from the default fixed-times
solve; the samples are mrs_tg_plan_sample's at dt.  Alternating within the run, in this order (the order --summarize relies on
to tell the variants of one kernel apart):
    sample_kernel<0>
    policy_validate_kernel               (launched through the library's internal launcher, which the shared object exports
                                          as a C++ symbol: max_deviation 0.2, first segment counted, no length gate)
    path_deviation_kernel "all"          every output
    path_deviation_kernel "policy"       the maximum and the segment maxima only: what policy_validate_kernel reports
    path_deviation_vjp_kernel            dL/dsamples and dL/dwaypoints
The timed families (kernel ids 8, 9) are timed by the library's own per-dispatch events; the other two are torch events around
the call (launch included) -- the rocprofv3 summary is the like-for-like kernel comparison.  Prints one JSON line per
configuration: medians in microseconds, the ratios, and the ballot rounds that explain the forward (per chunk of 64 samples:
the cursor advances in it plus one).
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402

VARIANTS = {"path_deviation_kernel": ("all", "policy")}
LAUNCH_POLICY_VALIDATE = "_ZN6mrs_tg22launch_policy_validateERKNS_18PolicyValidateArgsEP12ihipStream_t"


class PolicyValidateArgs(C.Structure):   # csrc/mrs_tg_launch.h
    _fields_ = [("n_paths", C.c_int), ("seg_offsets", C.c_void_p), ("wp", C.c_void_p), ("samples", C.c_void_p),
                ("n_samples", C.c_void_p), ("status", C.c_void_p), ("baca_total", C.c_void_p), ("dt", C.c_double),
                ("max_len_factor", C.c_double), ("min_len_factor", C.c_double), ("max_deviation", C.c_double),
                ("capacity", C.c_int), ("first_segment", C.c_int), ("check_enabled", C.c_int), ("last_round", C.c_int),
                ("ok_out", C.c_void_p), ("ns_out", C.c_void_p), ("status_out", C.c_void_p), ("max_dev_out", C.c_void_p),
                ("is_safe_out", C.c_void_p), ("safe_out", C.c_void_p), ("ns_copy", C.c_void_p)]


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
    samples = torch.zeros((P, cap, 4), dtype=torch.float64, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    dev, cur = torch.empty((P, cap), **f64), torch.empty((P, cap), **i32)
    mx, arg, seg = torch.empty(P, **f64), torch.empty(P, **i32), torch.empty(nS, **f64)
    G = torch.randn((P, cap), generator=torch.Generator(device="cuda").manual_seed(0), **f64)
    gs, gw = torch.empty((P, cap, 4), **f64), torch.empty((nS + P, 4), **f64)
    so = torch.from_numpy(np.ascontiguousarray(batch.seg_offsets, dtype=np.int32)).cuda()
    baca = torch.ones(P, **f64)
    ok, ns_out, st_out, ns_copy = (torch.empty(P, **i32) for _ in range(4))
    pmax = torch.empty(P, **f64)
    is_safe, safe = torch.empty(P, dtype=torch.uint8, device="cuda"), torch.empty(nS, dtype=torch.uint8, device="cuda")
    args = PolicyValidateArgs(P, so.data_ptr(), db.waypoints.data_ptr(), samples.data_ptr(), n_dev.data_ptr(), db.status.data_ptr(),
                              baca.data_ptr(), dt, 0.0, 0.0, 0.2, cap, 1, 1, 0, ok.data_ptr(), ns_out.data_ptr(), st_out.data_ptr(),
                              pmax.data_ptr(), is_safe.data_ptr(), safe.data_ptr(), ns_copy.data_ptr())
    launch_validate = getattr(api.load_library(), LAUNCH_POLICY_VALIDATE)
    launch_validate.restype = C.c_int
    launch_validate.argtypes = [C.POINTER(PolicyValidateArgs), C.c_void_p]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = OrderedDict((k, []) for k in ("sample", "validate", "dev_all", "dev_policy", "dev_vjp"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ev[0].record()
        plan.sample(db.coeffs, db.seg_times, dt, cap, n_dev, samples)
        ev[1].record()
        ev[2].record()
        rc = launch_validate(C.byref(args), stream)
        ev[3].record()
        assert rc == 0, rc
        ctx.set_profiling(True)
        got = OrderedDict()
        got["dev_all"] = timed(api.KERNEL_DEVIATION, lambda: plan.path_deviation(
            samples, n_dev, db.waypoints, first_segment=True, status=db.status, deviation=dev, cursor=cur, max_deviation=mx,
            argmax=arg, segment_max=seg))
        got["dev_policy"] = timed(api.KERNEL_DEVIATION, lambda: plan.path_deviation(
            samples, n_dev, db.waypoints, first_segment=True, status=db.status, max_deviation=mx, segment_max=seg))
        got["dev_vjp"] = timed(api.KERNEL_DEVIATION_VJP, lambda: plan.path_deviation_vjp(
            samples, n_dev, db.waypoints, G, status=db.status, grad_samples=gs, grad_waypoints=gw))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload)
            out["sample"].append(ev[0].elapsed_time(ev[1]))
            out["validate"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    # the two kernels agree (the maximum in bits, the safe flags), and the rounds the wavefront kernel took
    assert torch.equal(mx, pmax) and torch.equal(seg <= 0.2, safe.bool())
    c = cur.cpu().numpy()
    n = n_dev.cpu().numpy()
    chunks = rounds = 0
    worst = 0
    for p in range(P):
        k = int(n[p]) - 1
        for k0 in range(0, k, 64):
            row = c[p, k0:min(k0 + 64, k)]
            nxt = c[p, min(k0 + 64, k)] if k0 + 64 < k else row[-1]
            adv = int(max(nxt, row[-1]) - row[0])
            chunks += 1
            rounds += adv + 1
            worst = max(worst, adv + 1)
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(config="%dx%s" % (n_paths, n_seg), segments=nS, samples=int(n.sum()), per_path=cap, dt=dt, reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res["chunks"] = chunks
    res["ballot_rounds_per_chunk"] = round(rounds / max(chunks, 1), 2)
    res["most_rounds_in_a_chunk"] = worst
    res["scan_steps_per_lane_of_policy_validate"] = int(n.max()) - 1
    res["dev_policy_over_validate_event"] = round(med["dev_policy"] / med["validate"], 3)
    res["dev_all_over_sample_kernel0_event"] = round(med["dev_all"] / med["sample"], 2)
    res["dev_vjp_over_sample_kernel0_event"] = round(med["dev_vjp"] / med["sample"], 2)
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
        if not any(s in name for s in ("sample_kernel", "policy_validate", "path_deviation")):
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

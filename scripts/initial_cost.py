"""What the initial condition, the prepended waypoint and the prediction splice cost as plan steps.

    python scripts/initial_cost.py [--reps 11] [--configs 1024,10240] > profiles/initial_cost.txt

Per configuration P paths of 200 samples each (capacity 256), a 41-row prediction and k = 6: the five kinds of kernel timed by
the library's per-dispatch events (mrs_tg_set_profiling, medians of --reps runs, at least 9) -- the initial condition, the
prepend (three launches, first to last), the splice in place and out of place, and the three backward passes -- beside the host
functions api.prepare_initial_condition and api.splice_prediction looped over the same requests on this machine's CPU.  The
kernels only copy: the figures say what the steps add to a solve, not how fast they could be; no threshold is set on them.
Prints one JSON line per configuration, times in microseconds."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrs_uav_trajectory_generation_amd import api  # noqa: E402

N_ROWS, CAP, N_PRED, K = 200, 256, 41, 6
OFFSET = 2.0 * (0.2 * (K - 1.5) + 0.01)       # the middle of the bin of k = 6


def measure(ctx, P, reps):
    rng = np.random.default_rng(P)
    dev = "cuda"
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    pred_h = [rng.uniform(-9, 9, (P, N_PRED, 4)) for _ in range(4)]
    tracker_h = rng.uniform(-9, 9, (P, 4, 4))
    samples_h = rng.uniform(-9, 9, (P, CAP, 4))
    wp_h = rng.uniform(-9, 9, (2 * P, 4))
    flags, tracker, t_age, uav = d(np.full(P, 1, np.int32)), d(tracker_h), d(np.full(P, 0.1)), d(np.zeros((P, 4)))
    offs, vo, pred, n_pred = d(np.full(P, OFFSET)), d(np.arange(0, 2 * P + 1, 2, dtype=np.int32)), [d(a) for a in pred_h], d(np.full(P, N_PRED, np.int32))
    age, wp = d(np.full(P, 0.05)), d(wp_h)
    decision, k = torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
    block = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    offsets = torch.empty(P + 1, dtype=torch.int32, device=dev)
    rows = torch.empty((3 * P, 4), dtype=torch.float64, device=dev)
    n_in, samples = d(np.full(P, N_ROWS, np.int32)), d(samples_h)
    out, n_out = torch.empty_like(samples), torch.empty(P, dtype=torch.int32, device=dev)
    g_block, g_rows, g_out = d(rng.uniform(-1, 1, (P, 4, 4))), d(rng.uniform(-1, 1, (2 * P, 4))), d(rng.uniform(-1, 1, (P, CAP, 4)))
    g_tracker, g_uav = torch.empty_like(block), torch.empty((P, 4), dtype=torch.float64, device=dev)
    g_pred = [torch.empty((P, N_PRED, 4), dtype=torch.float64, device=dev) for _ in range(4)]
    g_wp, g_row = torch.empty_like(wp), torch.empty((P, 4), dtype=torch.float64, device=dev)
    g_samples = torch.empty_like(samples)
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    t = {name: [] for name in ("initial_condition", "prepend", "splice_in_place", "splice_out_of_place", "splice_vjp",
                               "initial_condition_vjp", "prepend_vjp")}

    def last(kernel_id):
        ctx.synchronize()
        return ctx.kernel_ms_history(kernel_id, 1)[-1]
    try:
        ctx.set_profiling(True)
        for rep in range(reps + 2):
            plan.initial_condition(flags, tracker, t_age, uav, 0.0, offs, vo, pred, n_pred, decision, k, block)
            a = last(api.KERNEL_INITIAL_CONDITION)
            plan.prepend_initial_condition(vo, wp, decision, block, offsets, rows)
            b = last(api.KERNEL_PREPEND_INITIAL_CONDITION)
            work, n_work = samples.clone(), n_in.clone()
            plan.splice_prediction(work, n_work, decision, k, age, pred[0], n_pred)
            c = last(api.KERNEL_SPLICE_PREDICTION)
            plan.splice_prediction(samples, n_in, decision, k, age, pred[0], n_pred, samples_out=out, n_samples_out=n_out)
            e = last(api.KERNEL_SPLICE_PREDICTION)
            plan.splice_prediction_vjp(n_in, decision, k, age, n_pred, g_out, g_samples, g_pred[0])
            f = last(api.KERNEL_SPLICE_PREDICTION_VJP)
            plan.initial_condition_vjp(decision, k, g_block, g_tracker, g_uav, g_pred)
            g = last(api.KERNEL_INITIAL_CONDITION_VJP)
            plan.prepend_initial_condition_vjp(vo, decision, offsets, g_rows, g_wp, g_row)
            h = last(api.KERNEL_PREPEND_INITIAL_CONDITION_VJP)
            if rep >= 2:                       # two warm-up rounds
                for name, v in zip(t, (a, b, c, e, f, g, h)):
                    t[name].append(v)
        ctx.set_profiling(False)
        assert int(k[0]) == K and int(n_out[0]) == N_ROWS + K and torch.equal(work[:, :N_ROWS + K], out[:, :N_ROWS + K])
    finally:
        plan.close()
    # the host functions, one request after the other
    host_prepare, host_splice = [], []
    for rep in range(reps):
        t0 = time.perf_counter()
        for p in range(P):
            tr = dict(position=tracker_h[p, 0], velocity=tracker_h[p, 1], acceleration=tracker_h[p, 2], jerk=tracker_h[p, 3])
            pr = dict(position=pred_h[0][p], velocity=pred_h[1][p], acceleration=pred_h[2][p], jerk=pred_h[3][p])
            api.prepare_initial_condition(tr, 0.1, pr, None, 0.0, OFFSET, 2, False)
        t1 = time.perf_counter()
        for p in range(P):
            pr = dict(position=pred_h[0][p], velocity=pred_h[1][p], acceleration=pred_h[2][p], jerk=pred_h[3][p])
            api.splice_prediction(pr, K, 0.05, samples_h[p, :N_ROWS], sample_capacity=CAP)
        host_splice.append(time.perf_counter() - t1)
        host_prepare.append(t1 - t0)
    res = dict(config="%dx%d" % (P, N_ROWS), reps=reps, k=K, pred_rows=N_PRED)
    res.update({name + "_us": round(float(np.median(v)) * 1e3, 2) for name, v in t.items()})
    res["host_prepare_loop_us"] = round(float(np.median(host_prepare)) * 1e6, 1)
    res["host_splice_loop_us"] = round(float(np.median(host_splice)) * 1e6, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--configs", default="1024,10240")
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit("medians of at least 9 runs")
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for P in (int(c) for c in a.configs.split(",")):
        print(json.dumps(measure(ctx, P, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

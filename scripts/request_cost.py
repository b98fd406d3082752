"""What the request's vertices cost as a plan step, beside the torch construction the step replaced.

    python scripts/request_cost.py [--reps 11] > profiles/request_cost.txt

Two batches: 4096 requests of 2 .. 11 waypoints (ragged) and 1024 requests of 10 segments (uniform), every request with an
initial state whose heading is a turn away from its first waypoint's.  Timed, medians of --reps runs (at least 9) after two
warm-up runs:
  request_vertices_kernel_us   the dispatch of Plan.request_vertices, by the library's per-dispatch events
  request_vertices_us          the same call between two events on the stream (launch overhead included)
  torch_construction_us        Plan.unwrap_headings + _unwrap_from_state + _vertices, the functions policy_steps had before this
                               step (copied below as the thing being replaced), between two events: one library launch and
                               about twenty small torch kernels; headings_with_other_bits: where its result differs from the
                               step's
  round_after_ms / round_before_ms   one round of policy_steps.optimize_paths (max_deviation_iterations = 0: thinning, one
                               round, the readback; host wall clock, the call ends synchronised) as it is, and with
                               Plan.request_vertices swapped for the old construction
No target is set on these figures.  Prints one JSON line per batch."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrs_uav_trajectory_generation_amd import api, policy_steps  # noqa: E402
from mrs_uav_trajectory_generation_amd import problem as pr  # noqa: E402


# ---- the construction this step replaced, as policy_steps had it -------------------------------------------------------------

def _vertices(so, unwrapped, stop, d, state=None):
    dev = unwrapped.device
    n_v = unwrapped.shape[0]
    first = torch.as_tensor(so[:-1] + np.arange(so.size - 1), dtype=torch.int64, device=dev)
    last = torch.as_tensor(so[1:] + np.arange(so.size - 1), dtype=torch.int64, device=dev)
    end = torch.zeros(n_v, dtype=torch.bool, device=dev)
    end[first] = True
    end[last] = True
    mask = torch.zeros((n_v, 5), dtype=torch.uint8, device=dev)
    mask[:, 0] = 1
    mask[:, 1:d + 1] = end[:, None].to(torch.uint8)
    mask[:, 1:4] |= ((stop != 0) & ~end)[:, None].to(torch.uint8)
    vals = torch.zeros((n_v, 5, api.N_DIM), dtype=torch.float64, device=dev)
    vals[:, 0, :] = unwrapped
    if state is not None:
        has, rows = state
        at = first[has]
        mask[at, 1:4] = 1
        vals[at, 1:4, :] = rows[has][:, 1:4, :]
    return mask, vals


def _unwrap_from_state(so, unwrapped, state):
    has, rows = state
    if not bool(has.any()):
        return
    dev = unwrapped.device
    first = torch.as_tensor(so[:-1] + np.arange(so.size - 1), dtype=torch.int64, device=dev)
    two_pi = 2.0 * np.pi

    def wrapped(x):
        return x - two_pi * torch.floor((x + np.pi) / two_pi)
    what, start = unwrapped[first, 3], rows[:, 0, 3]
    diff = wrapped(what) - wrapped(start)
    diff = torch.where(diff < -np.pi, diff + two_pi, torch.where(diff >= np.pi, diff - two_pi, diff))
    shift = torch.where(has & (what != start), start + diff - what, torch.zeros_like(what))
    counts = torch.as_tensor(np.diff(so).astype(np.int64) + 1, device=dev)
    unwrapped[:, 3] += torch.repeat_interleave(shift, counts, output_size=unwrapped.shape[0])


def old_request_vertices(plan, waypoints, waypoints_out=None, fixed_mask=None, fixed_values=None, stop_at=None, has_state=None,
                         state=None, derivative_to_optimize=4):
    """the signature of Plan.request_vertices over the old construction"""
    so = np.asarray(plan.seg_offsets_host, dtype=np.int64)
    plan.unwrap_headings(waypoints, waypoints_out)
    st = None if has_state is None else (has_state.to(torch.bool), state)
    if st is not None:
        _unwrap_from_state(so, waypoints_out, st)
    stop = stop_at if stop_at is not None else torch.zeros(waypoints.shape[0], dtype=torch.uint8, device=waypoints.device)
    mask, vals = _vertices(so, waypoints_out, stop, derivative_to_optimize, st)
    fixed_mask.copy_(mask)
    fixed_values.copy_(vals)


# ---- the measurement -------------------------------------------------------------------------------------------------------

def _requests(kind, rng):
    n = 4096 if kind == "ragged" else 1024
    paths, states = [], []
    for p in range(n):
        wp = pr.random_walk_waypoints(int(rng.integers(1, 11)) if kind == "ragged" else 10, 9000 + p)
        step = wp[1, :3] - wp[0, :3]
        vel = np.concatenate([rng.uniform(0.0, 1.5) * step / np.linalg.norm(step), [0.0]])
        paths.append(wp)
        states.append(dict(heading=float(wp[0, 3] + 4.0), velocity=vel, acceleration=np.zeros(4), jerk=np.zeros(4)))
    return paths, states


def _between_events(call, reps):
    out = []
    for rep in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if rep >= 2:
            out.append(a.elapsed_time(b))
    return float(np.median(out)) * 1e3


def measure(ctx, kind, reps):
    rng = np.random.default_rng(len(kind))
    paths, states = _requests(kind, rng)
    P, dev = len(paths), "cuda"
    so = np.concatenate([[0], np.cumsum([w.shape[0] - 1 for w in paths])]).astype(np.int32)
    wp = torch.from_numpy(np.concatenate(paths)).to(dev)
    n_v = wp.shape[0]
    rows = np.zeros((P, 4, 4))
    for p, st in enumerate(states):
        rows[p, 0, 3], rows[p, 1] = st["heading"], st["velocity"]
    rows = torch.from_numpy(rows).to(dev)
    has = torch.ones(P, dtype=torch.uint8, device=dev)
    stop = torch.zeros(n_v, dtype=torch.uint8, device=dev)
    out, mask = torch.empty_like(wp), torch.empty((n_v, 5), dtype=torch.uint8, device=dev)
    vals = torch.empty((n_v, 5, 4), dtype=torch.float64, device=dev)
    out2, mask2, vals2 = torch.empty_like(out), torch.empty_like(mask), torch.empty_like(vals)
    plan = api.Plan(ctx, so)
    plan.seg_offsets_host = so
    try:
        new = lambda: plan.request_vertices(wp, out, mask, vals, stop_at=stop, has_state=has, state=rows)           # noqa: E731
        old = lambda: old_request_vertices(plan, wp, out2, mask2, vals2, stop_at=stop, has_state=has, state=rows)   # noqa: E731
        ctx.set_profiling(True)
        kernel = []
        for rep in range(reps + 2):
            new()
            ctx.synchronize()
            if rep >= 2:
                kernel.append(ctx.kernel_ms_history(api.KERNEL_REQUEST_VERTICES, 1)[-1])
        ctx.set_profiling(False)
        t_new, t_old = _between_events(new, reps), _between_events(old, reps)
        differ = int((out[:, 3] != out2[:, 3]).sum())
        assert torch.equal(mask, mask2) and torch.equal(vals[:, 1:], vals2[:, 1:]) and torch.allclose(out, out2, rtol=0, atol=1e-14)
    finally:
        plan.close()
    policy = api.default_policy_options(solver=dict(derivative_to_optimize=4, sampling_dt=0.2), max_deviation_iterations=0)

    def one_round():
        t0 = time.perf_counter()
        policy_steps.optimize_paths(ctx, paths, policy=policy, sample_capacity=512, initial_states=states)
        return time.perf_counter() - t0
    after = [one_round() for _ in range(reps + 2)][2:]
    plan_init, real = api.Plan.__init__, api.Plan.request_vertices

    def init_keeping_offsets(self, c, seg_offsets):
        plan_init(self, c, seg_offsets)
        self.seg_offsets_host = np.asarray(seg_offsets)
    api.Plan.__init__, api.Plan.request_vertices = init_keeping_offsets, old_request_vertices
    try:
        before = [one_round() for _ in range(reps + 2)][2:]
    finally:
        api.Plan.__init__, api.Plan.request_vertices = plan_init, real
    return dict(config="%d %s, %d vertices" % (P, "x 2..11 waypoints" if kind == "ragged" else "x 10 segments", n_v), reps=reps,
                request_vertices_kernel_us=round(float(np.median(kernel)) * 1e3, 2), request_vertices_us=round(t_new, 1),
                torch_construction_us=round(t_old, 1), headings_with_other_bits=differ,
                round_after_ms=round(float(np.median(after)) * 1e3, 2), round_before_ms=round(float(np.median(before)) * 1e3, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit("medians of at least 9 runs")
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for kind in ("ragged", "uniform"):
        print(json.dumps(measure(ctx, kind, a.reps)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()

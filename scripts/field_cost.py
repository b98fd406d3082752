#!/usr/bin/env python3
"""What the clearance from a voxel distance field and its backward pass cost: field_clearance_kernel
(mrs_tg_plan_field_clearance, one workgroup per path, one lane per row, eight gathered voxels per row) and
field_clearance_vjp_kernel (mrs_tg_plan_field_clearance_vjp, one lane per row) against the torch composition of the same
trilinear lookup -- floor, clamp, eight gathers, seven lerps, a mask -- and its autograd backward, on the GPU.

    python scripts/field_cost.py [--reps 20] [--grids 64,256,512] [--paths 16,64,256,1024] [--rows 512] [--obstacles 1024,4096]

The rows come from real solves and samples: pr.random_batch's paths, solved with estimated times and sampled at the dt that
gives the longest path `--rows` rows, so that neighbouring rows of a path lie a fraction of a voxel to a few voxels apart (the
line says how many, on average).  The grid is a cube of n^3 nodes fitted round all samples; its values are the distance to
sixteen spheres, computed on the device slab by slab (what the field holds does not change what a lookup costs).  A batch of P
paths is the first P of the same samples.  Alternating within the run:
    field_clearance_kernel "all"       every output, the field's gradient included
    field_clearance_kernel "rows"      clearance, cell, minimum and argmin: what autograd.field_clearance asks for
    field_clearance_kernel "shuffled"  "rows" on the same rows in a random order within every path: what spatial coherence is worth
    field_clearance_vjp_kernel         dL/dsamples of sum(relu(R - clearance)), R the median clearance: half the rows are inside the hinge
    torch forward                      the composition, clearance and cell
    torch forward + backward           the same and .backward() of the same loss
and, as context, obstacle_clearance_kernel on the same rows against `--obstacles` random obstacles.
The kernels (ids 39, 40, 37) are timed by the library's own per-dispatch events; the composition is some forty launches, timed
by torch events around it, so its figure includes its launches' gaps -- which is what its user pays.  Prints one JSON line per
(grid, paths): medians in microseconds, the agreement of the two routes (clearance to 1e-12, cell exactly, the gradient to 1e-12
of its largest entry), rows per nanosecond and the bytes per second of voxel reads the forward sustains (64 bytes per inside row).
"""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api, problem as pr  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
I32 = dict(dtype=torch.int32, device="cuda")


def make_samples(ctx, n_paths, n_seg, rows):
    """(samples [P][cap][4], n [P] int32) of real solves: random_batch, estimated times, one solve, sampled so that the longest
    path has `rows` rows"""
    batch = pr.random_batch(n_paths, n_seg, seed0=0)
    plan = api.Plan(ctx, batch.seg_offsets)
    db = api.DeviceBatch(batch, "cuda:0")
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
               limits=db.limits)
    plan.solve(api.default_options(derivative_to_optimize=4), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status,
               db.cost)
    torch.cuda.synchronize()
    so = torch.from_numpy(np.asarray(batch.seg_offsets, dtype=np.int64)).cuda()
    total = torch.zeros(n_paths, **F64).index_add_(0, torch.repeat_interleave(torch.arange(n_paths, device="cuda"), so[1:] - so[:-1]),
                                                   db.seg_times)
    dt = float(total.max()) / (rows - 1.5)
    n = torch.zeros(n_paths, **I32)
    samples = torch.zeros((n_paths, rows, 4), **F64)
    plan.sample(db.coeffs, db.seg_times, dt, rows, n, samples)
    torch.cuda.synchronize()
    n = torch.clamp(n, max=rows).contiguous()
    assert bool(torch.all(db.status > 0)) and rows - 2 <= int(n.max()) <= rows, (int(n.max()), rows)
    plan.close()
    return samples, n


def make_field(geometry, seed):
    """[1][nz][ny][nx] on the device: the distance to sixteen spheres in the grid's box, slab by slab"""
    nx, ny, nz = geometry.dims
    o, h = geometry.origin, geometry.spacing
    gen = torch.Generator(device="cuda").manual_seed(seed)
    lo = torch.tensor(o, **F64)
    ext = torch.tensor([(n - 1) * s for n, s in zip(geometry.dims, h)], **F64)
    centre = lo + torch.rand((16, 3), generator=gen, **F64) * ext
    radius = 0.02 * float(ext.min()) * (1.0 + torch.rand(16, generator=gen, **F64))
    x = o[0] + torch.arange(nx, **F64) * h[0]
    y = o[1] + torch.arange(ny, **F64) * h[1]
    field = torch.empty((1, nz, ny, nx), **F64)
    for k in range(nz):
        z = o[2] + k * h[2]
        best = torch.full((ny, nx), float("inf"), **F64)
        for q in range(16):
            d = torch.sqrt((x[None, :] - centre[q, 0]) ** 2 + (y[:, None] - centre[q, 1]) ** 2 + (z - centre[q, 2]) ** 2) - radius[q]
            best = torch.minimum(best, d)
        field[0, k] = best
    return field


def torch_composition(rows, n, field, geometry):
    """(clearance [P][Q], cell [P][Q]) of the same lookup as a torch expression, differentiable in rows: +inf and -1 outside
    the grid and behind a path's last row"""
    nx, ny, nz = geometry.dims
    o = torch.tensor(geometry.origin, **F64)
    h = torch.tensor(geometry.spacing, **F64)
    top = torch.tensor([nx - 1.0, ny - 1.0, nz - 1.0], **F64)
    u = (rows[..., :3] - o) / h
    inside = ((u >= 0.0) & (u <= top)).all(dim=-1)
    idx = torch.minimum(torch.where(inside[..., None], u, torch.zeros_like(u)).detach().floor(), top - 1.0)
    t = u - idx
    i, j, k = (idx[..., a].long() for a in range(3))
    flat = field.reshape(-1)
    v = [flat[((k + K) * ny + (j + J)) * nx + (i + I)] for K in (0, 1) for J in (0, 1) for I in (0, 1)]
    c00, c10 = v[0] + t[..., 0] * (v[1] - v[0]), v[2] + t[..., 0] * (v[3] - v[2])
    c01, c11 = v[4] + t[..., 0] * (v[5] - v[4]), v[6] + t[..., 0] * (v[7] - v[6])
    c0, c1 = c00 + t[..., 1] * (c10 - c00), c01 + t[..., 1] * (c11 - c01)
    c = c0 + t[..., 2] * (c1 - c0)
    valid = inside & (torch.arange(rows.shape[1], device="cuda")[None, :] < n[:, None])
    return torch.where(valid, c, torch.full_like(c, float("inf"))), torch.where(valid, (k * ny + j) * nx + i, torch.full_like(i, -1))


def measure(ctx, samples, n, geometry, field, P, reps, obstacle_counts):
    rows, n = samples[:P].contiguous(), n[:P].contiguous()
    Q = rows.shape[1]
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    c, q, gr = torch.empty((P, Q), **F64), torch.empty((P, Q), **I32), torch.empty((P, Q, 4), **F64)
    mn, arg = torch.empty(P, **F64), torch.empty((P, 2), **I32)
    gs = torch.empty((P, Q, 4), **F64)
    gen = torch.Generator(device="cuda").manual_seed(7)
    # the same rows in a random order within every path (the rows behind a path's last stay behind it)
    key = torch.rand((P, Q), generator=gen, device="cuda") + (torch.arange(Q, device="cuda")[None, :] >= n[:, None]) * 2.0
    shuffled = rows[torch.arange(P, device="cuda")[:, None], key.argsort(dim=1)].contiguous()
    c_sh, q_sh = torch.empty((P, Q), **F64), torch.empty((P, Q), **I32)
    plan.field_clearance(rows, n, field, geometry, clearance=c, cell=q)
    radius = float(c[q >= 0].median())                        # the hinge takes half the rows, whatever the field holds
    up = -(c < radius).to(torch.float64)                      # dL/dclearance of sum(relu(radius - clearance))
    names = ["fwd_all", "fwd_rows", "fwd_rows_shuffled", "vjp", "torch_fwd", "torch_fwd_bwd"] + ["obstacles_%d" % m for m in obstacle_counts]
    out = OrderedDict((k, []) for k in names)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    obstacle_sets = []
    lo, hi = rows[..., :3].amin(dim=(0, 1)), rows[..., :3].amax(dim=(0, 1))
    for m in obstacle_counts:
        ob = torch.zeros((m, 4), **F64)
        ob[:, :3] = lo + torch.rand((m, 3), generator=gen, **F64) * (hi - lo)
        obstacle_sets.append((m, ob, torch.tensor([0, m], **I32)))
    oc, oq = torch.empty((P, Q), **F64), torch.empty((P, Q), **I32)

    def timed(kernel_id, call):
        call()
        return ctx.kernel_ms_history(kernel_id, 1)[-1:]

    for r in range(reps + 2):
        ctx.set_profiling(True)
        got = OrderedDict()
        got["fwd_all"] = timed(api.KERNEL_FIELD_CLEARANCE, lambda: plan.field_clearance(
            rows, n, field, geometry, clearance=c, cell=q, gradient=gr, min_clearance=mn, argmin=arg))
        got["fwd_rows"] = timed(api.KERNEL_FIELD_CLEARANCE, lambda: plan.field_clearance(
            rows, n, field, geometry, clearance=c, cell=q, min_clearance=mn, argmin=arg))
        got["fwd_rows_shuffled"] = timed(api.KERNEL_FIELD_CLEARANCE, lambda: plan.field_clearance(
            shuffled, n, field, geometry, clearance=c_sh, cell=q_sh, min_clearance=mn, argmin=arg))
        got["vjp"] = timed(api.KERNEL_FIELD_CLEARANCE_VJP, lambda: plan.field_clearance_vjp(rows, n, field, geometry, q, up, gs))
        for m, ob, off in obstacle_sets:
            got["obstacles_%d" % m] = timed(api.KERNEL_OBSTACLE_CLEARANCE, lambda: plan.obstacle_clearance(
                rows, n, ob, off, clearance=oc, nearest=oq))
        ctx.set_profiling(False)
        torch.cuda.synchronize()
        ev[0].record()
        with torch.no_grad():
            tc, tq = torch_composition(rows, n, field, geometry)
        ev[1].record()
        ev[2].record()
        leaf = rows.detach().requires_grad_(True)
        torch.relu(radius - torch_composition(leaf, n, field, geometry)[0]).sum().backward()
        ev[3].record()
        torch.cuda.synchronize()
        if r >= 2:   # (the first two rounds: code upload, the allocator's first blocks)
            out["torch_fwd"].append(ev[0].elapsed_time(ev[1]))
            out["torch_fwd_bwd"].append(ev[2].elapsed_time(ev[3]))
            for k, v in got.items():
                out[k] += v
    gt = leaf.grad
    inside = q >= 0
    live = torch.arange(Q, device="cuda")[None, :] < n[:, None]
    both = inside & (tq >= 0)
    agree = OrderedDict(clearance_max_abs_diff=float((c - tc)[both].abs().max()), cell_differ=int((q.long() != tq).sum()),
                        gradient_max_abs_diff=float((gs - gt).abs().max()), gradient_max_abs=float(gt.abs().max()),
                        least_clearance=float(c.min()), hinge_radius=round(radius, 3), rows_inside_the_hinge=int((c < radius).sum()))
    assert agree["clearance_max_abs_diff"] <= 1e-12 and agree["cell_differ"] == 0, agree
    assert agree["gradient_max_abs_diff"] <= 1e-12 * max(agree["gradient_max_abs"], 1e-300) and not bool(gs[..., 3].any()), agree
    assert bool(torch.equal(c_sh.sort(dim=1).values, c.sort(dim=1).values))          # the same rows, another order
    step = (rows[:, 1:, :3] - rows[:, :-1, :3]) / torch.tensor(geometry.spacing, **F64)
    pair = live[:, 1:] & live[:, :-1]
    plan.close()
    med = {k: float(np.median(v)) * 1e3 for k, v in out.items()}
    res = OrderedDict(grid=geometry.dims[0], field_MB=round(field.numel() * 8 / 1e6, 1), paths=P, capacity=Q,
                      live_rows=int(live.sum()), inside_rows=int(inside.sum()),
                      mean_step_in_voxels=round(float(step.norm(dim=-1)[pair].mean()), 3), reps=reps)
    for k, v in med.items():
        res[k + "_us"] = round(v, 2)
    res.update(agree)
    res["fwd_rows_inside_rows_per_ns"] = round(res["inside_rows"] / (med["fwd_rows"] * 1e3), 3)
    res["fwd_rows_voxel_GB_per_s"] = round(res["inside_rows"] * 64 / (med["fwd_rows"] * 1e-6) / 1e9, 1)
    res["shuffled_over_fwd_rows"] = round(med["fwd_rows_shuffled"] / med["fwd_rows"], 2)
    res["torch_fwd_over_fwd_rows"] = round(med["torch_fwd"] / med["fwd_rows"], 1)
    res["torch_fwd_bwd_over_fwd_rows_plus_vjp"] = round(med["torch_fwd_bwd"] / (med["fwd_rows"] + med["vjp"]), 1)
    res["library"] = os.path.basename(api.LIB_PATH)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grids", default="64,256,512")
    ap.add_argument("--paths", default="16,64,256,1024")
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--obstacles", default="1024,4096")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("field_cost.py measures on the GPU and found none")
    ctx = api.Context(0)
    ctx.use_torch_stream()
    paths = [int(p) for p in a.paths.split(",")]
    obstacle_counts = [int(m) for m in a.obstacles.split(",") if m]
    samples, n = make_samples(ctx, max(paths), a.segments, a.rows)
    live = torch.arange(a.rows, device="cuda")[None, :] < n[:, None]
    xyz = samples[..., :3]
    lo = torch.where(live[..., None], xyz, torch.full_like(xyz, float("inf"))).amin(dim=(0, 1))
    hi = torch.where(live[..., None], xyz, torch.full_like(xyz, float("-inf"))).amax(dim=(0, 1))
    margin = 0.01 * (hi - lo)
    for grid in (int(g) for g in a.grids.split(",")):
        spacing = ((hi - lo + 2.0 * margin) / (grid - 1)).tolist()
        geometry = api.FieldGeometry((lo - margin).tolist(), spacing, (grid, grid, grid), 1)
        field = make_field(geometry, 99)
        for P in paths:
            print(json.dumps(measure(ctx, samples, n, geometry, field, P, a.reps, obstacle_counts if grid == 64 else [])),
                  flush=True)
        del field
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

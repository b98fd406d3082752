#!/usr/bin/env python3
"""What the distance field from an occupancy grid costs: mrs_tg_field_from_occupancy (edt_x_kernel, edt_y_kernel, edt_z_kernel:
an exact Euclidean distance transform in three passes) against the two ways there were before, on the
same grid and in the same run, on the GPU.

    python scripts/edt_cost.py [--reps 20] [--grids 64,256,512] [--densities 0.001,0.02,0.3] [--caps inf,2.0] [--spacing 0.1]

The grid is a cube of n^3 nodes with the spacing `--spacing` on every axis and a random occupancy of the given density (seeded).
Alternating within the run, medians of `--reps` after two warm-up rounds:
    field_from_occupancy   the signed field, once per cap; id 41 of the library's per-dispatch events: the first launch's start
                           to the last launch's end (three launches, their two boundaries included)
    recipe                 section 11k's recipe: obstacle_clearance_kernel (id 37) with the nodes of one grid line as the rows
                           of one path, against the occupied voxels as points -- all of them where there are at most
                           `--recipe-points` (4096), else a random subset of that many (`recipe_points` and `recipe_is_subset`
                           say which: the subset's field is NOT the map's, its time is what that many points cost).  It builds
                           the unsigned field; `--recipe-reps` (5) repetitions, it is slow.
    scipy                  scipy.ndimage.distance_transform_edt of the occupancy and of its complement on the host (the signed
                           field needs both) and the copy of the result to the device, by the host clock around a synchronise;
                           up to `--scipy-max` (256) nodes per axis, `--scipy-reps` (3) repetitions; skipped where scipy is not
                           installed.  Its values are held to the device's to 1e-9 (its arithmetic is its own).
The floor: one read of the occupancy and one write of the field, 9 bytes per voxel, at the 6.3 TB/s a copy achieves on this
device (MI355X: 8 TB/s peak) -- `floor_us`, and `floor_fraction` = floor / measured.  What the three passes move by design: the
x pass reads 1 byte and writes 8 per voxel, the y and the z pass read and write 8 each (one array holds both transforms): 41
bytes per voxel -- `design_bytes_GB_per_s` is that over the measured time.
Prints one JSON line per (grid, density)."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api  # noqa: E402

F64 = dict(dtype=torch.float64, device="cuda")
I32 = dict(dtype=torch.int32, device="cuda")
COPY_BYTES_PER_S = 6.3e12            # what a copy achieves (of 8.0e12 peak)
FLOOR_BYTES_PER_VOXEL = 1 + 8
DESIGN_BYTES_PER_VOXEL_SIGNED = (1 + 8) + (8 + 8) + (8 + 8)


def node_rows(geometry):
    """[nz ny][nx][4] on the device: the nodes of one grid line as the rows of one path"""
    nx, ny, nz = geometry.dims
    o, h = geometry.origin, geometry.spacing
    rows = torch.zeros((nz, ny, nx, 4), **F64)
    rows[..., 0] = (o[0] + torch.arange(nx, **F64) * h[0])[None, None, :]
    rows[..., 1] = (o[1] + torch.arange(ny, **F64) * h[1])[None, :, None]
    rows[..., 2] = (o[2] + torch.arange(nz, **F64) * h[2])[:, None, None]
    return rows.reshape(nz * ny, nx, 4)


def measure(ctx, grid, density, caps, spacing, a):
    geometry = api.FieldGeometry((0.0, 0.0, 0.0), (spacing,) * 3, (grid,) * 3, 1)
    gen = torch.Generator(device="cuda").manual_seed(1000 + grid)
    occupancy = (torch.rand(geometry.fields_shape(), generator=gen, device="cuda") < density).to(torch.uint8)
    voxels = occupancy.numel()
    occupied = int(occupancy.sum())
    out = torch.empty(geometry.fields_shape(), **F64)
    times = OrderedDict(("edt_cap_%g" % cap, []) for cap in caps)
    for r in range(a.reps + 2):
        ctx.set_profiling(True)
        for cap in caps:
            ctx.field_from_occupancy(occupancy, geometry, max_distance=cap, out=out)
            ms = ctx.kernel_ms_history(api.KERNEL_FIELD_FROM_OCCUPANCY, 1)[-1:]
            if r >= 2:
                times["edt_cap_%g" % cap] += ms
        ctx.set_profiling(False)
    res = OrderedDict(grid=grid, density=density, voxels=voxels, occupied=occupied, field_MB=round(voxels * 8 / 1e6, 1),
                      spacing=spacing, reps=a.reps)
    floor_us = voxels * FLOOR_BYTES_PER_VOXEL / COPY_BYTES_PER_S * 1e6
    res["floor_us"] = round(floor_us, 2)
    for k, v in times.items():
        us = float(np.median(v)) * 1e3
        res[k + "_us"] = round(us, 1)
        res[k + "_spread_us"] = [round(float(np.min(v)) * 1e3, 1), round(float(np.max(v)) * 1e3, 1)]
        res[k + "_floor_fraction"] = round(floor_us / us, 4)
        res[k + "_design_bytes_GB_per_s"] = round(voxels * DESIGN_BYTES_PER_VOXEL_SIGNED / (us * 1e-6) / 1e9, 1)
    # the field every yardstick is held to: unsigned, no cap
    unsigned = ctx.field_from_occupancy(occupancy, geometry, signed=False)
    signed = ctx.field_from_occupancy(occupancy, geometry)
    torch.cuda.synchronize()
    # section 11k's recipe over the nodes
    points_index = occupancy.reshape(-1).nonzero().reshape(-1)
    subset = occupied > a.recipe_points
    if subset:
        points_index = points_index[torch.randperm(occupied, generator=gen, device="cuda")[:a.recipe_points]].sort().values
    rows = node_rows(geometry)
    points = rows.reshape(-1, 4)[points_index].contiguous()
    res["recipe_points"], res["recipe_is_subset"] = int(points.shape[0]), bool(subset)
    if points.shape[0] > 0:
        lines = api.Plan(ctx, np.arange(grid * grid + 1, dtype=np.int32))
        count = torch.full((grid * grid,), grid, **I32)
        offsets = torch.tensor([0, points.shape[0]], **I32)
        recipe = torch.empty((grid * grid, grid), **F64)
        got = []
        for r in range(a.recipe_reps + 1):
            ctx.set_profiling(True)
            lines.obstacle_clearance(rows, count, points, offsets, clearance=recipe)
            ms = ctx.kernel_ms_history(api.KERNEL_OBSTACLE_CLEARANCE, 1)[-1:]
            ctx.set_profiling(False)
            if r >= 1:
                got += ms
        lines.close()
        res["recipe_us"] = round(float(np.median(got)) * 1e3, 1)
        res["recipe_over_edt"] = round(res["recipe_us"] / res["edt_cap_%g_us" % caps[0]], 1)
        if not subset:   # the same map: the same field to rounding (the recipe subtracts coordinates, the transform counts voxels)
            res["recipe_max_abs_diff"] = float((recipe.reshape(unsigned.shape) - unsigned).abs().max())
            assert res["recipe_max_abs_diff"] <= 1e-9 * grid * spacing, res
        del recipe
    del rows
    # the host route
    if grid <= a.scipy_max:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            host = occupancy.cpu().numpy()[0] != 0
            got = []
            for r in range(a.scipy_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                field = ndimage.distance_transform_edt(~host, sampling=(spacing,) * 3) - ndimage.distance_transform_edt(host, sampling=(spacing,) * 3)
                t1 = time.perf_counter()
                dev = torch.from_numpy(field).cuda()
                torch.cuda.synchronize()
                got.append((t1 - t0, time.perf_counter() - t1))
            res["scipy_host_us"] = round(float(np.median([g[0] for g in got])) * 1e6, 1)
            res["scipy_copy_us"] = round(float(np.median([g[1] for g in got])) * 1e6, 1)
            res["scipy_over_edt"] = round((res["scipy_host_us"] + res["scipy_copy_us"]) / res["edt_cap_%g_us" % caps[0]], 1)
            if 0 < occupied < voxels:
                res["scipy_max_abs_diff"] = float((dev[None] - signed).abs().max())
                assert res["scipy_max_abs_diff"] <= 1e-9 * grid * spacing, res
    res["library"] = os.path.basename(api.LIB_PATH)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grids", default="64,256,512")
    ap.add_argument("--densities", default="0.001,0.02,0.3")
    ap.add_argument("--caps", default="inf,2.0")
    ap.add_argument("--spacing", type=float, default=0.1)
    ap.add_argument("--recipe-points", type=int, default=4096)
    ap.add_argument("--recipe-reps", type=int, default=5)
    ap.add_argument("--scipy-max", type=int, default=256)
    ap.add_argument("--scipy-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edt_cost.py measures on the GPU and found none")
    ctx = api.Context(0)
    ctx.use_torch_stream()
    caps = [float(c) for c in a.caps.split(",")]
    for grid in (int(g) for g in a.grids.split(",")):
        for density in (float(d) for d in a.densities.split(",")):
            print(json.dumps(measure(ctx, grid, density, caps, a.spacing, a)), flush=True)
            torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

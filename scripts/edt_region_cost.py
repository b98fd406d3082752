#!/usr/bin/env python3
"""What bringing the distance field up to date after a change inside a box costs: mrs_tg_field_update_region
(edt_region_x_kernel, edt_region_y_kernel, edt_region_z_kernel: the three passes on a window of the grid, DESIGN.md section
11m) against the full rebuild mrs_tg_field_from_occupancy of the same grid, in the same run, on the GPU.

    python scripts/edt_region_cost.py [--reps 20] [--grids 256,512] [--boxes 8,32,64] [--caps 1.0,2.0] [--density 0.02] [--spacing 0.1]

The grid is a cube of n^3 nodes with the spacing `--spacing` on every axis and a random occupancy of the given density (seeded),
the field signed.  Per cap, box edge and place (the grid's centre, the corner at node 0): the box is rerandomised at density
0.5, the field updated once and held to the rebuild of the new occupancy bit for bit; then, alternating within the run, medians
of `--reps` after two warm-up rounds, both by id 41 of the library's per-dispatch events (the first launch's start to the last
launch's end):
    update   field_update_region of that box with a workspace allocated once
    full     field_from_occupancy of the same grid
Prints one JSON line per case: the reach, the core's and the window's voxel counts, the window's share of the grid, the
workspace, both times and update / full."""
import argparse
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mrs_uav_trajectory_generation_amd import api  # noqa: E402


def extent(lo, hi):
    return int(np.prod([h - l + 1 for l, h in zip(lo, hi)]))


def measure(ctx, grid, occupancy, geometry, cap, edge, place, a):
    lo = (0, 0, 0) if place == "corner" else ((grid - edge) // 2,) * 3
    hi = tuple(l + edge - 1 for l in lo)
    info = api.field_update_query(geometry, lo, hi, max_distance=cap)
    gen = torch.Generator(device="cuda").manual_seed(grid + edge)
    new = occupancy.clone()
    new[0, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = (torch.rand((edge,) * 3, generator=gen, device="cuda") < 0.5).to(torch.uint8)
    workspace = torch.empty((max(info["workspace_bytes"] // 8, 1),), dtype=torch.float64, device="cuda")
    field = ctx.field_from_occupancy(occupancy, geometry, max_distance=cap)
    before = field.clone()
    api.kernel_trace_reset()
    ctx.field_update_region(new, field, geometry, lo, hi, max_distance=cap, workspace=workspace)
    kernels = api.kernel_trace()
    rebuilt = ctx.field_from_occupancy(new, geometry, max_distance=cap)
    torch.cuda.synchronize()
    assert torch.equal(field.view(torch.int64), rebuilt.view(torch.int64)), "the update is not the rebuild"
    changed = int((before.view(torch.int64) != field.view(torch.int64)).sum())
    del before
    times = dict(update=[], full=[])
    for r in range(a.reps + 2):
        ctx.set_profiling(True)
        ctx.field_update_region(new, field, geometry, lo, hi, max_distance=cap, workspace=workspace)
        update = ctx.kernel_ms_history(api.KERNEL_FIELD_FROM_OCCUPANCY, 1)[-1:]
        ctx.field_from_occupancy(new, geometry, max_distance=cap, out=rebuilt)
        full = ctx.kernel_ms_history(api.KERNEL_FIELD_FROM_OCCUPANCY, 1)[-1:]
        ctx.set_profiling(False)
        if r >= 2:
            times["update"] += update
            times["full"] += full
    voxels = grid ** 3
    window = extent(info["window_lo"], info["window_hi"])
    res = OrderedDict(grid=grid, cap=cap, box=edge, place=place, reach=info["reach"], whole_grid=info["whole_grid"],
                      kernels=kernels[0] if kernels else None, core_voxels=extent(info["core_lo"], info["core_hi"]),
                      window_voxels=window, window_share=round(window / voxels, 5),
                      workspace_MB=round(info["workspace_bytes"] / 1e6, 2), nodes_changed=changed, reps=a.reps)
    for k, v in times.items():
        res[k + "_us"] = round(float(np.median(v)) * 1e3, 1)
        res[k + "_spread_us"] = [round(float(np.min(v)) * 1e3, 1), round(float(np.max(v)) * 1e3, 1)]
    res["update_over_full"] = round(res["update_us"] / res["full_us"], 4)
    res["library"] = os.path.basename(api.LIB_PATH)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grids", default="256,512")
    ap.add_argument("--boxes", default="8,32,64")
    ap.add_argument("--caps", default="1.0,2.0")
    ap.add_argument("--density", type=float, default=0.02)
    ap.add_argument("--spacing", type=float, default=0.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edt_region_cost.py measures on the GPU and found none")
    ctx = api.Context(0)
    ctx.use_torch_stream()
    for grid in (int(g) for g in a.grids.split(",")):
        geometry = api.FieldGeometry((0.0, 0.0, 0.0), (a.spacing,) * 3, (grid,) * 3, 1)
        gen = torch.Generator(device="cuda").manual_seed(1000 + grid)
        occupancy = (torch.rand(geometry.fields_shape(), generator=gen, device="cuda") < a.density).to(torch.uint8)
        for cap in (float(c) for c in a.caps.split(",")):
            for edge in (int(b) for b in a.boxes.split(",")):
                for place in ("centre", "corner"):
                    print(json.dumps(measure(ctx, grid, occupancy, geometry, cap, edge, place, a)), flush=True)
                    torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

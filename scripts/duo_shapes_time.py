"""Time of ONE launch of the two-sided solve (solve_duo_kernel) at shapes the headline does not run: a uniform batch, a ragged
batch sorted by length (uniform wavefronts next to mixed ones) and a ragged batch in drawn order (mixed wavefronts only: the
predicated loops and the plain stores).  Median over 30 timed groups of 20 launches (events), microseconds per launch.
  MRS_TG_LIB_PATH=.../libmrs_tg_NAME.so python scripts/duo_shapes_time.py     # compare builds on one box, alternating"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrs_uav_trajectory_generation_amd import api, problem as pr


def ragged(n, lo, hi, seed, sort):
    segs = [lo + (pr.SplitMix64(seed + p).next_u64() % (hi - lo + 1)) for p in range(n)]
    if sort:
        segs.sort()
    parts = [pr.build_vertices(pr.random_box_waypoints(S, seed + 100000 + p), pr.SNAP) for p, S in enumerate(segs)]
    return pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (n, 1)))


def main():
    ctx = api.Context(0)
    ctx.use_torch_stream()
    shapes = [("8192 x 10 uniform", pr.random_batch(8192, 10, seed0=300)),
              ("8192 x 7..12 sorted", ragged(8192, 7, 12, 500, True)),
              ("8192 x 7..12 drawn order", ragged(8192, 7, 12, 500, False))]
    for name, batch in shapes:
        plan = api.Plan(ctx, batch.seg_offsets)
        db = api.DeviceBatch(batch, "cuda:0")
        est = api.default_options(derivative_to_optimize=4, estimate_times=1)
        plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
                   limits=db.limits)
        call = plan.bind_solve(api.default_options(derivative_to_optimize=4), db.fixed_mask, db.fixed_values, db.seg_times,
                               db.coeffs, db.status, db.cost, waypoints=db.waypoints)
        api.kernel_trace_reset()
        call()
        kern = api.kernel_trace()[-1]
        for _ in range(200):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                call()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b) * 1e3 / 20)
        print("%-26s %-26s median %.2f us  min %.2f  max %.2f" % (name, kern, np.median(t), min(t), max(t)))
        plan.close()
    ctx.close()


if __name__ == "__main__":
    main()

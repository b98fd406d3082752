"""The device blocks a plan allocates on first use (csrc/mrs_tg_block.hpp: every one is a DeviceBlock of its plan), route by
route, through the existing API only.  Per route: the call on plan A twice (the second finds every block held), A destroyed, a
plan B of the same shape (whose blocks are A's, recycled by the pool) once more.  The three calls give the same bits, and so
does the whole sequence in a child process under MRS_TG_POOL_POISON=1 (every block handed out is filled with 0xFF first; the
knob is read once per process): no route reads a block it did not fill, a block filled once when allocated is filled again
on the next plan, and a block that grows is replaced behind a synchronise.

Every route here is bit-reproducible between two calls (the sequence passes on the commit before the owner type as well), so
the comparison is equality, without a tolerance.

The routes, at the smallest shapes that reach them: Mellinger with FLAG_CAREFUL_COST 64 x 10 (with careful_count); the
gradient-free modes 0 and 3, 16 x 4; FLAG_GENERAL_PATTERNS with one position-free vertex in modes -1 and 2, 16 x 5;
FLAG_MATERIALIZED_BLOCKS 32 x 5; the plan's workspace growing call by call (default solve, FLAG_REFINE, solve_vjp, a bound
group of two: 3072 x 4, where two batches make the 6144 paths from which the grouped dispatch takes the kernel that uses the
workspace); preprocess_path then insert_midpoints, 8 x 6; Mellinger on 40960 x 3, a uniform batch of more workgroups than the
device holds at once, so that the lean kernel claims its paths from the queue counter (set_queue_kernel in the trace)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api, problem as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _start_times(batch):
    """a start point for the segment times from the waypoints alone: half the segment's length plus half a second"""
    d = np.linalg.norm(np.diff(batch.waypoints[:, :3], axis=0), axis=1)
    so = batch.seg_offsets
    seams = [int(so[p + 1]) + p for p in range(batch.n_paths - 1)]   # the "segment" from a path's last vertex to the next path's first
    return 0.5 * np.delete(d, seams) + 0.5


def _solve(plan, db, t0, **opts):
    import torch
    db.seg_times.copy_(torch.from_numpy(t0))
    for t in (db.coeffs, db.status, db.cost):
        t.zero_()
    plan.solve(api.default_options(**opts), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost,
               waypoints=db.waypoints, limits=db.limits)
    torch.cuda.synchronize()
    return dict(coeffs=db.coeffs.cpu().numpy(), times=db.seg_times.cpu().numpy(), cost=db.cost.cpu().numpy(),
                status=db.status.cpu().numpy())


def _solver_route(batch, with_careful_count=False, **opts):
    def call(plan, db):
        out = _solve(plan, db, _start_times(batch), **opts)
        if with_careful_count:
            out["careful_count"] = np.array([plan.careful_count()])
        return out
    return batch, call


def _one_position_free_vertex(batch):
    mask = batch.fixed_mask.copy()
    mask[int(batch.seg_offsets[3]) + 3 + 2, 0] = 0   # vertex 2 of path 3
    return pr.Batch(batch.seg_offsets, batch.waypoints, mask, batch.fixed_values, batch.limits, batch.derivative_to_optimize)


def _workspace_growth():
    import torch
    batch = pr.random_batch(3072, 4, seed0=11)
    other = pr.random_batch(3072, 4, seed0=12)
    rng = np.random.default_rng(5)
    G, g = rng.standard_normal((batch.n_segments, 4, 10)), rng.standard_normal(batch.n_paths)

    def call(plan, db):
        t0 = _start_times(batch)
        out = {"plain_" + k: v for k, v in _solve(plan, db, t0).items()}
        out.update({"refine_" + k: v for k, v in _solve(plan, db, t0, flags=api.FLAG_REFINE).items()})
        gv, gt = torch.zeros_like(db.fixed_values), torch.zeros_like(db.seg_times)
        plan.solve_vjp(4, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, torch.from_numpy(G).cuda(),
                       torch.from_numpy(g).cuda(), gv, gt)
        torch.cuda.synchronize()
        out.update(vjp_values=gv.cpu().numpy(), vjp_times=gt.cpu().numpy())
        db2 = api.DeviceBatch(other, "cuda:0")
        db2.seg_times.copy_(torch.from_numpy(_start_times(other)))
        db.coeffs.zero_()
        lin = api.default_options()
        calls = [plan.bind_solve(lin, d.fixed_mask, d.fixed_values, d.seg_times, d.coeffs, d.status, d.cost) for d in (db, db2)]
        api.RoundRobin(calls, grouped=True)(2)
        torch.cuda.synchronize()
        for k, d in enumerate((db, db2)):
            out.update({"group%d_coeffs" % k: d.coeffs.cpu().numpy(), "group%d_cost" % k: d.cost.cpu().numpy(),
                        "group%d_status" % k: d.status.cpu().numpy()})
        return out
    return batch, call


def _path_edit():
    import torch
    batch = pr.random_batch(8, 6, seed0=21)
    V, S, P = batch.waypoints.shape[0], batch.n_segments, batch.n_paths
    seg_max = np.where(np.arange(S) % 3 == 0, 0.5, 0.01)

    def call(plan, db):
        out = {}
        for name, rows in (("thin", V), ("subdivide", V + S)):
            offsets = torch.zeros(P + 1, dtype=torch.int32, device="cuda")
            wp_out = torch.zeros((rows, 4), dtype=torch.float64, device="cuda")
            source = torch.zeros(rows, dtype=torch.int32, device="cuda")
            if name == "thin":
                plan.preprocess_path(db.waypoints, offsets, wp_out, min_waypoint_distance=1.0, source=source)
            else:
                plan.insert_midpoints(db.waypoints, torch.from_numpy(seg_max).cuda(), 0.1, offsets, wp_out, source=source)
            torch.cuda.synchronize()
            out.update({name + "_offsets": offsets.cpu().numpy(), name + "_waypoints": wp_out.cpu().numpy(),
                        name + "_source": source.cpu().numpy()})
        return out
    return batch, call


NO_LIMITS = np.full(9, 1e9)  # feasibility scaling off: the returned times are the outer loop's own
ROUTES = {
    "mellinger_careful": lambda: _solver_route(pr.random_batch(64, 10, seed0=0, limits=NO_LIMITS), with_careful_count=True,
                                               time_alloc_method=api.TIME_ALLOC_MELLINGER, flags=api.FLAG_CAREFUL_COST),
    "gradient_free_mode0": lambda: _solver_route(pr.random_batch(16, 4, seed0=1), time_alloc_method=0),
    "gradient_free_mode3": lambda: _solver_route(pr.random_batch(16, 4, seed0=1), time_alloc_method=3),
    "general_fixed_times": lambda: _solver_route(_one_position_free_vertex(pr.random_batch(16, 5, seed0=2)),
                                                 flags=api.FLAG_GENERAL_PATTERNS),
    "general_mellinger": lambda: _solver_route(_one_position_free_vertex(pr.random_batch(16, 5, seed0=2)),
                                               time_alloc_method=api.TIME_ALLOC_MELLINGER, flags=api.FLAG_GENERAL_PATTERNS),
    "materialized_blocks": lambda: _solver_route(pr.random_batch(32, 5, seed0=3), flags=api.FLAG_MATERIALIZED_BLOCKS),
    "workspace_growth": _workspace_growth,
    "path_edit": _path_edit,
    "queued_lean": lambda: _solver_route(pr.random_batch(40960, 3, seed0=4), time_alloc_method=api.TIME_ALLOC_MELLINGER),
}


def run_routes(ctx):
    """{route: [what the call gave on plan A, on plan A again, on plan B]}, and the kernel names of queued_lean's last call"""
    results = {}
    for name, make in ROUTES.items():
        batch, call = make()
        db = api.DeviceBatch(batch, "cuda:0")
        results[name] = []
        for n_calls in (2, 1):   # plan A, then plan B of the same shape
            plan = api.Plan(ctx, batch.seg_offsets)
            try:
                for _ in range(n_calls):
                    api.kernel_trace_reset()
                    results[name].append(call(plan, db))
            finally:
                plan.close()
    return results, api.kernel_trace()


def _child(path):
    ctx = api.Context(0)
    ctx.use_torch_stream()
    results, trace = run_routes(ctx)
    ctx.close()
    np.savez(path, trace=np.array(trace), **{"%s/%d/%s" % (route, k, key): a for route, calls in results.items()
                                            for k, out in enumerate(calls) for key, a in out.items()})


@pytest.fixture(scope="module")
def runs(gpu_ctx, tmp_path_factory):
    """the sequence in this process, and in a child under MRS_TG_POOL_POISON=1; computed once, read by every test"""
    plain, trace = run_routes(gpu_ctx)
    path = str(tmp_path_factory.mktemp("plan_blocks") / "poisoned.npz")
    subprocess.run([sys.executable, "-m", "tests.test_gpu_plan_blocks", "--child", path], check=True, cwd=ROOT, timeout=600,
                   env=dict(os.environ, MRS_TG_POOL_POISON="1"))
    z = np.load(path)
    poisoned = {route: [{key: z["%s/%d/%s" % (route, k, key)] for key in out} for k, out in enumerate(calls)]
                for route, calls in plain.items()}
    return dict(plain=plain, poisoned=poisoned, trace=trace, poisoned_trace=[str(s) for s in z["trace"]])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("route", list(ROUTES))
def test_held_recycled_and_poisoned_blocks_give_the_same_bits(runs, route):
    first = runs["plain"][route][0]
    for key, a in first.items():
        if a.dtype.kind == "f":
            assert np.all(np.isfinite(a)), key
        if key.endswith("status"):
            assert np.all(a >= 1), key
    for kind in ("plain", "poisoned"):
        for k, out in enumerate(runs[kind][route]):
            assert out.keys() == first.keys()
            for key, a in first.items():
                assert _same_bits(out[key], a), (kind, ("plan A", "plan A again", "plan B")[k], key)


def test_the_queued_launch_ran(runs):
    assert "set_queue_kernel" in runs["trace"] and "set_queue_kernel" in runs["poisoned_trace"], runs["trace"]


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])

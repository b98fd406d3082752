"""The backward pass of the fixed-times solve on the GPU (mrs_tg_plan_solve_vjp, vjp_kernel) and the autograd Function built on
it (mrs_uav_trajectory_generation_amd.autograd.solve):

  * the capability bit; the 60-digit fixtures through the ABI at the CPU tier's bounds, and the GPU equal to the CPU harness
    (tests/host/vjp_harness.cpp) to 1e-13 on the same inputs;
  * torch.autograd.gradcheck of the Function in fixed_values and seg_times on a 4-path batch;
  * against the dense float64 torch restatement (tests/vjp_util.py): 1024 x 10 at d = 2, 3, 4 and the 8192-path mixed /
    ragged batch with stop_at and position-free vertices added;
  * the Function's forward equals Plan.solve bit for bit; backward on a non-default stream equals the default stream; two
    identical calls give identical bits; a poisoned pool (MRS_TG_POOL_POISON=1, a child process) changes nothing;
  * a path with status -2 gets zero rows and leaves the others' bits alone; NULL arguments are MRS_TG_ERR_INVALID_ARG.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from tests import util
from tests import vjp_util as vu

pytestmark = pytest.mark.gpu

TOL_WELL, TOL_ILL, ILL_CASE = 1e-10, 1e-5, "ratio50"   # the CPU tier's bounds (test_vjp_host.py)
TOL_GPU_CPU = 1e-13
# against the dense torch restatement, whose own error dominates (a dense solve of the unscaled KKT system; measured on an
# MI355X: median 2e-8, p99 3e-7, max 7e-5 over these batches)
TOL_TORCH_MEDIAN, TOL_TORCH_P99, TOL_TORCH_MAX = 1e-7, 1e-5, 1e-3
GENERAL = api.FLAG_GENERAL_PATTERNS


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _vjp(plan, d, mask, vals, times, coeffs, status, G, g, want_values=True, want_times=True):
    gv = torch.full(tuple(vals.shape), float("nan"), dtype=torch.float64, device="cuda") if want_values else None
    gt = torch.full(tuple(times.shape), float("nan"), dtype=torch.float64, device="cuda") if want_times else None
    plan.solve_vjp(d, mask, vals, times, coeffs, status, grad_coeffs=G, grad_cost=g, grad_fixed_values=gv, grad_seg_times=gt)
    torch.cuda.synchronize()
    return (None if gv is None else gv.cpu().numpy()), (None if gt is None else gt.cpu().numpy())


def _solve(plan, d, db_mask, db_vals, times, flags=GENERAL):
    nS, P = plan.n_segments, plan.n_paths
    t = times.clone()
    coeffs = torch.zeros((nS, 4, 10), dtype=torch.float64, device="cuda")
    status = torch.zeros(P, dtype=torch.int32, device="cuda")
    cost = torch.zeros(P, dtype=torch.float64, device="cuda")
    plan.solve(api.default_options(derivative_to_optimize=d, flags=flags), db_mask, db_vals, t, coeffs, status, cost)
    return t, coeffs, status, cost


def test_the_library_reports_the_capability():
    assert api.capabilities() & api.CAP_GRADIENT
    assert api.CAP_GRADIENT == 8


def test_fixtures_through_the_abi_and_the_cpu_harness(gpu_ctx, tmp_path):
    cases = vu.load_cases()
    exe = vu.build_harness(tmp_path)
    cpu = vu.run_harness(exe, [vu.case_problem(c) for c in cases])
    rows = []
    for case, (cv, ct) in zip(cases, cpu):
        p = vu.case_problem(case)
        S = len(p["times"])
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            gv, gt = _vjp(plan, p["d"], _dev(p["mask"]), _dev(p["vals"]), _dev(p["times"]), _dev(p["coeffs"]),
                          _dev(np.ones(1, np.int32)), _dev(p["G"]), _dev(np.array([p["g"]])))
        finally:
            plan.close()
        gv = gv.reshape(S + 1, 5, 4)
        assert np.all(np.isfinite(gv)) and np.all(np.isfinite(gt)), case["name"]
        vs_cpu = vu.rel_error(gv, gt, cv, ct)
        if "directions" in case:
            e = vu.directional_error(case, gv, gt)
        else:
            e = vu.rel_error(gv, gt, np.array(case["grad_fixed_values"]), np.array(case["grad_seg_times"]))
        rows.append((case["name"], e, vs_cpu))
        assert e <= (TOL_ILL if case["name"] == ILL_CASE else TOL_WELL), rows[-1]
        assert vs_cpu <= TOL_GPU_CPU, rows[-1]
    print("VJP GPU FIXTURES (name, vs 60 digits, vs CPU harness): %s" % ["%s %.1e %.1e" % r for r in rows])


def _small_batch(n_paths=4, S=4, seed=50000):
    batch = pr.random_batch(n_paths, S, seed0=seed)
    return batch, util.oracle_times(batch)


def test_gradcheck_of_the_autograd_function(gpu_ctx):
    batch, t = _small_batch()
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    fv = _dev(batch.fixed_values).requires_grad_(True)
    times = _dev(t).requires_grad_(True)

    def f(v, tt):
        coeffs, cost, _ = autograd.solve(plan, mask, v, tt)
        return coeffs, cost
    try:
        # (eps 1e-4: the solve is exactly linear in the values, and the cost's rounding, ~1e-12 of its terms, stays far below
        # the tolerance; the central difference's truncation in the times is ~1e-8)
        assert torch.autograd.gradcheck(f, (fv, times), eps=1e-4, atol=1e-5, rtol=1e-3)
    finally:
        plan.close()


def _with_extra_patterns(batch):
    """stop_at vertices are in random_mixed_batch already; every seventh path with two or more segments also gets a vertex
    whose position is free"""
    m = batch.fixed_mask.copy()
    v = batch.fixed_values.copy()
    for p in range(batch.n_paths):
        v0, v1 = batch.vertex_range(p)
        if p % 7 == 0 and v1 - v0 >= 3:
            m[v0 + 1, 0] = 0
            v[v0 + 1, 0, :] = 0.0
    return pr.Batch(batch.seg_offsets, batch.waypoints, m, v, batch.limits, batch.derivative_to_optimize)


def _against_torch(ctx, batch, times, d, seed):
    P, so = batch.n_paths, batch.seg_offsets
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((batch.n_segments, 4, 10))
    g = rng.standard_normal(P)
    plan = api.Plan(ctx, so)
    try:
        mask, vals = _dev(batch.fixed_mask), _dev(batch.fixed_values)
        t, coeffs, status, cost = _solve(plan, d, mask, vals, _dev(times))
        gv, gt = _vjp(plan, d, mask, vals, t, coeffs, status, _dev(G), _dev(g))
    finally:
        plan.close()
    st = status.cpu().numpy()
    assert np.all(st == 1)
    S_of = np.diff(so)
    errs = np.zeros(P)
    for S in np.unique(S_of):
        idx = np.nonzero(S_of == S)[0]
        sel = batch.select(idx)
        segs = np.concatenate([np.arange(so[p], so[p + 1]) for p in idx])
        verts = np.concatenate([np.arange(*batch.vertex_range(p)) for p in idx])
        k = len(idx)
        _, _, rv, rt = vu.dense_vjp(sel.fixed_mask.reshape(k, S + 1, 5), sel.fixed_values.reshape(k, S + 1, 5, 4),
                                    times[segs].reshape(k, S), d, G[segs].reshape(k, S, 4, 10), g[idx])
        hv, ht = gv[verts].reshape(k, S + 1, 5, 4), gt[segs].reshape(k, S)
        for j, p in enumerate(idx):
            assert np.all(hv[j][sel.fixed_mask.reshape(k, S + 1, 5)[j] == 0] == 0.0), p
            errs[p] = vu.rel_error(hv[j], ht[j], rv[j], rt[j])
    return errs


def _report(label, errs):
    print("VJP GPU vs TORCH %s: %d paths, max %.2e, p99 %.2e, median %.2e" % (label, errs.size, errs.max(), np.quantile(errs, 0.99),
                                                                            np.median(errs)))


@pytest.mark.parametrize("d", [2, 3, 4])
def test_1024x10_against_the_torch_restatement(gpu_ctx, d):
    batch = pr.random_batch(1024, 10, seed0=51000 + d, derivative_to_optimize=d)
    errs = _against_torch(gpu_ctx, batch, util.oracle_times(batch), d, d)
    _report("1024x10 d=%d" % d, errs)
    assert np.all(np.isfinite(errs))
    assert np.median(errs) <= TOL_TORCH_MEDIAN and np.quantile(errs, 0.99) <= TOL_TORCH_P99 and errs.max() <= TOL_TORCH_MAX


def test_mixed_ragged_8192_against_the_torch_restatement(gpu_ctx):
    batch = _with_extra_patterns(pr.random_mixed_batch(8192, seed0=52000))
    errs = _against_torch(gpu_ctx, batch, util.oracle_times(batch), 4, 7)
    _report("mixed 8192", errs)
    assert np.all(np.isfinite(errs))
    assert np.median(errs) <= TOL_TORCH_MEDIAN and np.quantile(errs, 0.99) <= TOL_TORCH_P99 and errs.max() <= TOL_TORCH_MAX


def _loss_grads(plan, mask, fv0, t0, G, g, stream=None):
    fv = fv0.clone().requires_grad_(True)
    tt = t0.clone().requires_grad_(True)
    s = stream if stream is not None else torch.cuda.default_stream()
    s.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(s):
        coeffs, cost, status = autograd.solve(plan, mask, fv, tt)
        loss = (coeffs * G).sum() + (cost * g).sum()
        loss.backward()
    torch.cuda.synchronize()
    return coeffs.detach().cpu().numpy(), fv.grad.cpu().numpy(), tt.grad.cpu().numpy()


def test_forward_equals_plan_solve_and_streams_and_repeats_give_the_same_bits(gpu_ctx):
    batch = pr.random_batch(1024, 10, seed0=53000)
    t = _dev(util.oracle_times(batch))
    mask, fv = _dev(batch.fixed_mask), _dev(batch.fixed_values)
    rng = np.random.default_rng(11)
    G, g = _dev(rng.standard_normal((batch.n_segments, 4, 10))), _dev(rng.standard_normal(batch.n_paths))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        _, c_ref, st_ref, cost_ref = _solve(plan, 4, mask, fv, t)
        coeffs, cost, status = autograd.solve(plan, mask, fv, t)
        torch.cuda.synchronize()
        assert torch.equal(coeffs, c_ref) and torch.equal(cost, cost_ref) and torch.equal(status, st_ref)
        a = _loss_grads(plan, mask, fv, t, G, g)
        b = _loss_grads(plan, mask, fv, t, G, g)
        side = torch.cuda.Stream()
        c = _loss_grads(plan, mask, fv, t, G, g, stream=side)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.all(np.isfinite(a[1])) and np.any(a[2] != 0.0)


POISON_CHILD = r"""
import sys
sys.path.insert(0, %r)
import numpy as np, torch
from mrs_uav_trajectory_generation_amd import api, problem as pr
from tests import util
ctx = api.Context(0)
ctx.use_torch_stream()
batch = pr.random_batch(512, "ragged", seed0=54000)
t = torch.from_numpy(util.oracle_times(batch)).cuda()
rng = np.random.default_rng(12)
G = torch.from_numpy(rng.standard_normal((batch.n_segments, 4, 10))).cuda()
g = torch.from_numpy(rng.standard_normal(batch.n_paths)).cuda()
plan = api.Plan(ctx, batch.seg_offsets)
mask, fv = torch.from_numpy(batch.fixed_mask).cuda(), torch.from_numpy(batch.fixed_values).cuda()
coeffs = torch.zeros((batch.n_segments, 4, 10), dtype=torch.float64, device="cuda")
status = torch.zeros(batch.n_paths, dtype=torch.int32, device="cuda")
tt = t.clone()
plan.solve(api.default_options(flags=api.FLAG_GENERAL_PATTERNS), mask, fv, tt, coeffs, status)
gv = torch.zeros_like(fv)
gt = torch.zeros_like(t)
for _ in range(2):   # (the second call runs on recycled, poisoned blocks as well)
    plan.solve_vjp(4, mask, fv, tt, coeffs, status, G, g, gv, gt)
torch.cuda.synchronize()
np.save(sys.argv[1], np.concatenate([gv.cpu().numpy().reshape(-1), gt.cpu().numpy()]))
plan.close()
ctx.close()
"""


def test_a_poisoned_pool_changes_nothing(gpu_ctx, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_plain, out_poison = str(tmp_path / "plain.npy"), str(tmp_path / "poison.npy")
    for out, env in ((out_plain, {}), (out_poison, {"MRS_TG_POOL_POISON": "1"})):
        subprocess.run([sys.executable, "-c", POISON_CHILD % root, out], check=True, cwd=root, timeout=600, capture_output=True,
                       text=True, env=dict(os.environ, **env))
    a, b = np.load(out_plain), np.load(out_poison)
    assert np.all(np.isfinite(a)) and np.array_equal(a, b)


def test_a_path_with_status_minus_2_gets_zero_rows_and_leaves_the_others_alone(gpu_ctx):
    batch = pr.random_batch(64, "ragged", seed0=55000)
    t = util.oracle_times(batch)
    rng = np.random.default_rng(13)
    G, g = rng.standard_normal((batch.n_segments, 4, 10)), rng.standard_normal(batch.n_paths)
    bad = 17
    so = batch.seg_offsets

    plan = api.Plan(gpu_ctx, so)
    try:
        _, coeffs, status, _ = _solve(plan, 4, _dev(batch.fixed_mask), _dev(batch.fixed_values), _dev(t))
        torch.cuda.synchronize()
    finally:
        plan.close()
    coeffs, status = coeffs.cpu().numpy(), status.cpu().numpy()
    assert np.all(status == 1)

    def run(b, times, cb, stb, Gb, gb):
        plan = api.Plan(gpu_ctx, b.seg_offsets)
        try:
            return _vjp(plan, 4, _dev(b.fixed_mask), _dev(b.fixed_values), _dev(times), _dev(cb), _dev(stb), _dev(Gb), _dev(gb))
        finally:
            plan.close()
    st_bad = status.copy()
    st_bad[bad] = -2
    gv, gt = run(batch, t, coeffs, st_bad, G, g)
    v0, v1 = batch.vertex_range(bad)
    assert np.all(gv[v0:v1] == 0.0) and np.all(gt[so[bad]:so[bad + 1]] == 0.0)
    keep = [p for p in range(batch.n_paths) if p != bad]
    segs = np.concatenate([np.arange(so[p], so[p + 1]) for p in keep])
    verts = np.concatenate([np.arange(*batch.vertex_range(p)) for p in keep])
    rv, rt = run(batch.select(keep), t[segs], coeffs[segs], status[keep], G[segs], g[keep])
    assert np.array_equal(gv[verts], rv) and np.array_equal(gt[segs], rt)


def test_null_arguments_are_invalid(gpu_ctx):
    batch, t = _small_batch()
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        mask, vals = _dev(batch.fixed_mask), _dev(batch.fixed_values)
        tt, coeffs, status, _ = _solve(plan, 4, mask, vals, _dev(t))
        G = torch.zeros_like(coeffs)
        g = torch.ones(batch.n_paths, dtype=torch.float64, device="cuda")
        gv, gt = torch.zeros_like(vals), torch.zeros_like(tt)
        full = [plan._h, 4, mask, vals, tt, coeffs, status, G, g, gv, gt]
        L = gpu_ctx._L

        def call(args):
            return L.mrs_tg_plan_solve_vjp(*[a if not isinstance(a, torch.Tensor) else C.c_void_p(a.data_ptr()) for a in args])
        assert call(full) == 0
        for i in range(2, 7):   # the forward's inputs and outputs are required
            args = list(full)
            args[i] = None
            assert call(args) == -1, i
        for pair in ((7, 8), (9, 10)):   # at least one upstream and one output
            args = list(full)
            args[pair[0]] = args[pair[1]] = None
            assert call(args) == -1, pair
        for d in (-1, 5):
            args = list(full)
            args[1] = d
            assert call(args) == -1 and "derivative_to_optimize" in L.mrs_tg_last_error(gpu_ctx._h).decode()
        assert L.mrs_tg_plan_solve_vjp(None, 4, *([None] * 9)) == -1
        # one upstream and one output suffice: grad_cost alone, values only
        args = list(full)
        args[7] = None
        args[10] = None
        assert call(args) == 0
        torch.cuda.synchronize()
        assert torch.all(torch.isfinite(gv))
        # the dispatch is timed as kernel id 3
        gpu_ctx.set_profiling(True)
        assert call(full) == 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_VJP) > 0.0
        gpu_ctx.set_profiling(False)
    finally:
        plan.close()

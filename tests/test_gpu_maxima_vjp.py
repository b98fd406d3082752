"""The backward pass of the segment maxima on the GPU (mrs_tg_plan_segment_maxima_vjp, segment_maxima_vjp_kernel) and the
autograd pieces built on it (autograd.segment_maxima, autograd.scale_times_to_limits):

  * the capability bit; the 60-digit fixtures through the ABI (gradients to 1e-10, t* to 1e-12 T) and the GPU equal to the
    CPU harness (tests/host/maxima_vjp_harness.cpp) seeded with the GPU's t*, to 1e-12; the tie case equals one of its two
    one-sided gradients, with the same bits on two calls;
  * 10 240 x 10 and the 8192-path mixed / ragged batch: every t* in [0, T], |p^(k)(t*)| in torch equal to the forward's maxima
    (the backward pass followed the forward's winner) and the gradients equal to torch autograd of |p^(k)(t*)|;
  * determinism across streams and repeated calls; zero upstream, zero maxima, T <= 0; NULL arguments; kernel id 4 is timed;
  * the chain solve -> scale_times_to_limits -> solve -> L against the 60-digit composite fixtures
    (tests/golden/maxima_vjp_composite_cases.json): scale 1 and active v, a and j terms, an ill-conditioned path; a path with
    status <= 0 and non-finite coefficients keeps its times and gets zero, finite gradients;
  * scale_times_to_limits against a numpy restatement of violation_scaling (2 ulp); gradcheck of segment_maxima (times and
    coefficients of orders 0..4) and of the chain solve -> scale_times_to_limits -> solve on a small batch whose winners are
    separated by >= 1e-3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from tests import maxima_vjp_util as mu
from tests import util

pytestmark = pytest.mark.gpu

# (GPU vs CPU: the harness is seeded with the GPU's refined t*, not its seed, so the last Newton step may differ: measured
# 2.3e-13 on an MI355X)
TOL_FIX_GRAD, TOL_FIX_T, TOL_GPU_CPU = 1e-10, 1e-12, 1e-12
# |p^(k)(t*)| against the forward: relative to the larger of the value and the evaluation's own magnitude sum (an entry far
# below its polynomial's terms cancels, in torch's physical-time powers as in the kernel's normalised Horner)
# (the forward stops polishing at a 3e-7 abscissa step, which bounds its value to 1e-10, mrs_tg_maxima.hpp; measured 2.1e-12 and
# 5.4e-12 on the two batches below; 2e-11 still tells a wrong winner that is close in value)
TOL_SCALE = 2e-11
# gradients against torch autograd, relative to the segment's largest gradient component
TOL_SCALE_GRAD = 1e-10
GENERAL = api.FLAG_GENERAL_PATTERNS


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _seg_plan(ctx, n):
    return api.Plan(ctx, np.arange(n + 1, dtype=np.int32))


def _mvjp(plan, coeffs, times, G):
    nS = coeffs.shape[0]
    gc = torch.full((nS, 4, 10), float("nan"), dtype=torch.float64, device="cuda")
    gt = torch.full((nS,), float("nan"), dtype=torch.float64, device="cuda")
    am = torch.full((nS, 3, 3), float("nan"), dtype=torch.float64, device="cuda")
    plan.segment_maxima_vjp(coeffs, times, G, grad_coeffs=gc, grad_seg_times=gt, argmax=am)
    torch.cuda.synchronize()
    return gc, gt, am


def _solve(plan, batch, times, d=4):
    coeffs = torch.zeros((plan.n_segments, 4, 10), dtype=torch.float64, device="cuda")
    status = torch.zeros(plan.n_paths, dtype=torch.int32, device="cuda")
    cost = torch.zeros(plan.n_paths, dtype=torch.float64, device="cuda")
    t = times.clone()
    opt = api.default_options(derivative_to_optimize=d, time_alloc_method=api.TIME_ALLOC_NONE, estimate_times=0, sampling_dt=0.0,
                              flags=GENERAL)
    plan.solve(opt, _dev(batch.fixed_mask), _dev(batch.fixed_values), t, coeffs, status, cost)
    torch.cuda.synchronize()
    assert torch.all(status == 1)
    return coeffs


def test_the_library_reports_the_capability():
    assert api.capabilities() & api.CAP_MAXIMA_GRADIENT
    assert api.CAP_MAXIMA_GRADIENT == 16 and api.KERNEL_MAXIMA_VJP == 4


def test_fixtures_through_the_abi_and_the_cpu_harness(gpu_ctx, tmp_path):
    cases = mu.load_cases()
    n = 9 * len(cases)   # one copy of every segment per entry, upstream one-hot on that entry
    c = np.array([cs["coeffs"] for cs in cases for _ in range(9)])
    T = np.array([cs["T"] for cs in cases for _ in range(9)])
    G = np.tile(np.eye(9), (len(cases), 1)).reshape(n, 3, 3)
    plan = _seg_plan(gpu_ctx, n)
    try:
        gc, gt, am = _mvjp(plan, _dev(c), _dev(T), _dev(G))
        gc2, gt2, am2 = _mvjp(plan, _dev(c), _dev(T), _dev(G))
    finally:
        plan.close()
    gc, gt, am = gc.cpu().numpy(), gt.cpu().numpy(), am.cpu().numpy().reshape(n, 9)
    assert np.array_equal(gc, gc2.cpu().numpy()) and np.array_equal(gt, gt2.cpu().numpy())
    assert np.array_equal(am, am2.cpu().numpy().reshape(n, 9))
    exe = mu.build_harness(tmp_path)
    probs = []
    for ci, case in enumerate(cases):
        for w in range(9):
            taus = list(am[9 * ci + w] / case["T"])
            probs.append(mu.one_hot_problems(case, taus)[w])
    cpu = mu.run_harness(exe, probs)
    worst = dict(grad=0.0, t=0.0, cpu=0.0)
    for ci, case in enumerate(cases):
        for w, e in enumerate(case["entries"]):
            r = 9 * ci + w
            assert np.all(np.isfinite(gc[r])) and np.isfinite(gt[r]) and np.all(np.isfinite(am[r])), (case["name"], w)
            refs = e.get("alternatives", [e])
            errs = [(abs(am[r][w] - a["t"]) / case["T"], mu.entry_error(gc[r], gt[r], a) if e["maximum"] > 0 else
                     float(np.max(np.abs(gc[r])) + abs(gt[r]))) for a in refs]
            et, eg = min(errs, key=lambda x: x[1])
            ccg, cgt, cts = cpu[r]
            scale = max(np.max(np.abs(ccg)), abs(cgt), 1e-300)
            ec = max(np.max(np.abs(gc[r] - ccg)), abs(gt[r] - cgt)) / scale
            worst = dict(grad=max(worst["grad"], eg), t=max(worst["t"], et), cpu=max(worst["cpu"], ec))
            assert eg <= TOL_FIX_GRAD, (case["name"], w, eg)
            assert et <= TOL_FIX_T, (case["name"], w, et)
            assert ec <= TOL_GPU_CPU, (case["name"], w, ec)
    print("MAXIMA VJP GPU FIXTURES: gradients %.1e, t* %.1e T, GPU vs CPU %.1e" % (worst["grad"], worst["t"], worst["cpu"]))


def _scale_check(ctx, batch, times_np, seed):
    rng = np.random.default_rng(seed)
    plan = api.Plan(ctx, batch.seg_offsets)
    try:
        times = _dev(times_np)
        coeffs = _solve(plan, batch, times)
        nS = plan.n_segments
        maxima = torch.empty((nS, 3, 3), dtype=torch.float64, device="cuda")
        plan.segment_maxima(coeffs, times, maxima)
        G = _dev(rng.standard_normal((nS, 3, 3)))
        gc, gt, am = _mvjp(plan, coeffs, times, G)
    finally:
        plan.close()
    T = times.unsqueeze(1)
    t9 = am.reshape(nS, 9)
    assert torch.all(torch.isfinite(t9)) and torch.all(t9 >= 0.0) and torch.all(t9 <= T)
    # the backward pass followed the forward's winner: |p^(k)| at its t* is the forward's value
    M = mu.magnitudes_at(torch, coeffs, am)
    A = mu.magnitudes_at(torch, coeffs.abs(), am, absolute=True)
    rel_m = ((M - maxima).abs() / torch.maximum(maxima, A)).max().item()
    # the gradients: torch autograd of sum G |p^(k)(t*)|, t* held fixed except at the segment's end (where t* = T moves with T)
    c = coeffs.clone().requires_grad_(True)
    Tv = times.clone().requires_grad_(True)
    at_end = t9 == T
    t_used = torch.where(at_end, Tv.unsqueeze(1).expand(-1, 9), t9)
    L = (G * mu.magnitudes_at(torch, c, t_used.reshape(nS, 3, 3))).sum()
    L.backward()
    scale = torch.maximum(c.grad.abs().reshape(nS, -1).amax(dim=1), Tv.grad.abs())
    rel_g = torch.maximum((gc - c.grad).abs().reshape(nS, -1).amax(dim=1), (gt - Tv.grad).abs()) / scale.clamp_min(1e-300)
    return rel_m, rel_g.max().item()


@pytest.mark.parametrize("which", ["10240x10", "mixed8192"])
def test_scale_batches_follow_the_forward_winner_and_match_torch(gpu_ctx, which):
    if which == "10240x10":
        batch = pr.random_batch(10240, 10, seed0=61000)
    else:
        batch = pr.random_mixed_batch(8192, seed0=62000)
    rel_m, rel_g = _scale_check(gpu_ctx, batch, util.oracle_times(batch), 5)
    print("MAXIMA VJP %s: |p^(k)(t*)| vs forward %.1e, gradients vs torch %.1e" % (which, rel_m, rel_g))
    assert rel_m <= TOL_SCALE and rel_g <= TOL_SCALE_GRAD


def test_streams_repeats_zero_upstream_zero_maxima_and_bad_times(gpu_ctx):
    cases = mu.load_cases()
    const = next(c for c in cases if c["name"] == "constant_heading")
    c = np.array([cs["coeffs"] for cs in cases] * 3)
    T = np.array([cs["T"] for cs in cases] * 3)
    n = len(T)
    T[1], T[2] = 0.0, -2.0                                    # zero rows
    rng = np.random.default_rng(3)
    G = rng.standard_normal((n, 3, 3))
    G[3] = 0.0                                                # an all-zero upstream segment
    plan = _seg_plan(gpu_ctx, n)
    try:
        a = _mvjp(plan, _dev(c), _dev(T), _dev(G))
        b = _mvjp(plan, _dev(c), _dev(T), _dev(G))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            gpu_ctx.use_torch_stream()
            s = _mvjp(plan, _dev(c), _dev(T), _dev(G))
        gpu_ctx.use_torch_stream()
        # only the zero-maximum heading entries of the constant-heading segment carry an upstream
        ci = next(i for i, cs in enumerate(cases) if cs is const)
        Gh = np.zeros((n, 3, 3))
        Gh[ci, :, 2] = 1.0
        h = _mvjp(plan, _dev(c), _dev(T), _dev(Gh))
    finally:
        plan.close()
    for x, y, z in zip(a, b, s):
        assert torch.equal(x, y) and torch.equal(x, z)
    gc, gt, am = [x.cpu().numpy() for x in a]
    assert np.all(np.isfinite(gc)) and np.all(np.isfinite(gt))
    for r in (1, 2):
        assert np.all(gc[r] == 0.0) and gt[r] == 0.0 and np.all(am[r] == 0.0)
    assert np.all(gc[3] == 0.0) and gt[3] == 0.0
    hc, ht, _ = [x.cpu().numpy() for x in h]
    assert np.all(hc == 0.0) and np.all(ht == 0.0)


def test_null_arguments_are_invalid_and_the_kernel_is_timed(gpu_ctx):
    cases = mu.load_cases()
    c = _dev(np.array([cs["coeffs"] for cs in cases]))
    T = _dev(np.array([cs["T"] for cs in cases]))
    n = len(cases)
    G = torch.ones((n, 3, 3), dtype=torch.float64, device="cuda")
    gc = torch.zeros((n, 4, 10), dtype=torch.float64, device="cuda")
    gt = torch.zeros(n, dtype=torch.float64, device="cuda")
    am = torch.zeros((n, 3, 3), dtype=torch.float64, device="cuda")
    plan = _seg_plan(gpu_ctx, n)
    L = gpu_ctx._L
    try:
        full = [plan._h, c, T, G, gc, gt, am]

        def call(args):
            return L.mrs_tg_plan_segment_maxima_vjp(*[C.c_void_p(x.data_ptr()) if isinstance(x, torch.Tensor) else x for x in args])
        assert call(full) == 0
        for i in (1, 2, 3):
            args = list(full)
            args[i] = None
            assert call(args) == -1, i
        args = list(full)
        args[4] = args[5] = args[6] = None
        assert call(args) == -1
        assert L.mrs_tg_plan_segment_maxima_vjp(None, *([None] * 6)) == -1
        for keep in (4, 5, 6):   # any one output suffices
            args = list(full)
            for i in (4, 5, 6):
                if i != keep:
                    args[i] = None
            assert call(args) == 0
        gpu_ctx.set_profiling(True)
        assert call(full) == 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_MAXIMA_VJP) > 0.0
        gpu_ctx.set_profiling(False)
        torch.cuda.synchronize()
    finally:
        plan.close()


def test_scale_times_to_limits_matches_violation_scaling(gpu_ctx):
    batch = pr.random_mixed_batch(2048, seed0=63000)
    times = util.oracle_times(batch)
    lim = batch.limits * np.random.default_rng(4).uniform(0.2, 1.5, batch.limits.shape)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        coeffs = _solve(plan, batch, _dev(times))
        status = torch.ones(plan.n_paths, dtype=torch.int32, device="cuda")
        status[::5] = -2
        scaled = autograd.scale_times_to_limits(plan, coeffs, _dev(times), _dev(lim), status).cpu().numpy()
        maxima = torch.empty((plan.n_segments, 3, 3), dtype=torch.float64, device="cuda")
        plan.segment_maxima(coeffs, _dev(times), maxima)
        mx = maxima.cpu().numpy().reshape(-1, 9)
    finally:
        plan.close()
    path = np.repeat(np.arange(batch.n_paths), np.diff(batch.seg_offsets))
    ref = times * mu.violation_scaling_np(mx, lim[path])
    st = np.ones(batch.n_paths, dtype=bool)
    st[::5] = False
    ref = np.where(st[path], ref, times)
    ulp = np.abs(scaled - ref) / np.spacing(ref)
    print("SCALE vs violation_scaling: max %.1f ulp, %d of %d segments scaled" % (ulp.max(), np.sum(ref != times), ref.size))
    assert ulp.max() <= 2.0
    assert np.any(ref != times) and np.all(scaled[~st[path]] == times[~st[path]])


def _separated(coeffs, times, min_gap=1e-3, n=4097):
    """per segment: the best and second-best local maxima of every non-zero entry differ by >= min_gap relative (dense torch
    sampling: the winner does not change under gradcheck's perturbations)"""
    nS = coeffs.shape[0]
    tau = torch.linspace(0.0, 1.0, n, dtype=torch.float64, device=coeffs.device)
    t = (times.unsqueeze(1) * tau).unsqueeze(1).expand(nS, 9, n)
    ok = torch.ones(nS, dtype=torch.bool, device=coeffs.device)
    for w in range(9):
        k, grp = w // 3 + 1, w % 3
        m = torch.zeros((nS, n), dtype=torch.float64, device=coeffs.device)
        for i in range(0, n, 512):
            p = mu.derivative_at(torch, coeffs, t[:, :, i:i + 512].reshape(nS, -1), k).reshape(nS, 9, -1, 4)[:, w]
            m[:, i:i + 512] = torch.sqrt((p[..., list(mu.GROUPS[grp])] ** 2).sum(-1))
        pad = torch.full((nS, 1), -1.0, dtype=torch.float64, device=coeffs.device)
        mp_ = torch.cat([pad, m, pad], dim=1)
        peak = (m >= mp_[:, :-2]) & (m > mp_[:, 2:]) | (m > mp_[:, :-2]) & (m >= mp_[:, 2:])
        vals = torch.where(peak, m, torch.zeros_like(m)).sort(dim=1, descending=True).values
        best, second = vals[:, 0], vals[:, 1]
        ok &= (best == 0) | (best - second >= min_gap * best)
    return ok


def test_gradcheck_of_segment_maxima_and_of_the_feasibility_chain(gpu_ctx):
    batch = pr.random_batch(6, 3, seed0=64000)
    times_np = util.oracle_times(batch)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        times = _dev(times_np)
        coeffs = _solve(plan, batch, times)
        sep = _separated(coeffs, times)
        assert torch.all(sep), sep
        maxima = torch.empty((plan.n_segments, 3, 3), dtype=torch.float64, device="cuda")
        plan.segment_maxima(coeffs, times, maxima)
        # in the times and the coefficients of orders 0..4 (the higher ones move p^(k) by t^(j-k) eps, 1e6 eps at j = 9 on
        # these 5 s segments: a finite difference that large no longer sees the first-order term)
        lo = coeffs[..., :5].clone().requires_grad_(True)
        hi = coeffs[..., 5:].clone()
        tt = times.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: autograd.segment_maxima(plan, torch.cat([a, hi], dim=-1), b), (lo, tt),
                                        eps=1e-6, atol=1e-5, rtol=1e-3)
        # limits: only the horizontal velocity is active, every segment's ratio >= 1.25 (a 25 % margin over 1 and over the
        # other terms, which are far below their limits)
        mx = maxima.cpu().numpy().reshape(-1, 9)
        path = np.repeat(np.arange(batch.n_paths), np.diff(batch.seg_offsets))
        lim = np.full((batch.n_paths, 9), 1e6)
        for p in range(batch.n_paths):
            lim[p, 0] = 0.8 * mx[path == p, 0].min()
        mask = _dev(batch.fixed_mask)
        fv = _dev(batch.fixed_values).requires_grad_(True)
        lt = _dev(lim).requires_grad_(True)
        rng = np.random.default_rng(9)
        Gc = _dev(rng.standard_normal((plan.n_segments, 4, 10)))
        w = _dev(rng.standard_normal((plan.n_segments, 3, 3)))

        def chain(v, t0, li):
            c1, _, st = autograd.solve(plan, mask, v, t0)
            t1 = autograd.scale_times_to_limits(plan, c1, t0, li, st)
            c2, _, _ = autograd.solve(plan, mask, v, t1)
            return (Gc * c2).sum() + (w * autograd.segment_maxima(plan, c2, t1)).sum()
        assert torch.autograd.gradcheck(chain, (fv, times.clone().requires_grad_(True), lt), eps=1e-6, atol=1e-5, rtol=1e-3)
    finally:
        plan.close()


TOL_COMPOSITE = 1e-9
ILL_COMPOSITE = "composite_ill_short_segment"
# the 0.05 s segment between 5 s ones: measured 1.7e-8, the cond * eps of its solves
TOL_COMPOSITE_ILL = 5e-8


def test_the_feasibility_chain_matches_the_composite_fixtures(gpu_ctx):
    cases = mu.load_composite_cases()
    assert {i for c in cases for i in c["active"]} == {0, 1, 2, 3}   # scale 1, and v, sqrt a, cbrt j active
    errs = {}
    for case in cases:
        S = len(case["seg_times"])
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            mask = _dev(np.array(case["fixed_mask"], dtype=np.uint8))
            fv = _dev(np.array(case["fixed_values"])).requires_grad_(True)
            t0 = _dev(np.array(case["seg_times"])).requires_grad_(True)
            lim = _dev(np.array(case["limits"])[None])
            G, w = _dev(np.array(case["G"])), _dev(np.array(case["w"]))
            d = case["derivative_to_optimize"]
            c1, _, st = autograd.solve(plan, mask, fv, t0, derivative=d)
            t1 = autograd.scale_times_to_limits(plan, c1, t0, lim, st)
            c2, _, _ = autograd.solve(plan, mask, fv, t1, derivative=d)
            L = (G * c2).sum() + (w * autograd.segment_maxima(plan, c2, t1)).sum()
            L.backward()
            torch.cuda.synchronize()
            ts = t1.detach().cpu().numpy()
            gv, gt = fv.grad.cpu().numpy(), t0.grad.cpu().numpy()
        finally:
            plan.close()
        rv, rt = np.array(case["grad_fixed_values"]), np.array(case["grad_seg_times"])
        scale = max(np.max(np.abs(rv)), np.max(np.abs(rt)))
        t_err = np.max(np.abs(ts - case["scaled_times"]) / np.array(case["scaled_times"]))
        errs[case["name"]] = (max(np.max(np.abs(gv - rv)), np.max(np.abs(gt - rt))) / scale, t_err)
    print("MAXIMA VJP COMPOSITE (gradients, scaled times): %s" % {k: "%.1e %.1e" % v for k, v in errs.items()})
    for name, e in errs.items():
        assert max(e) <= (TOL_COMPOSITE_ILL if name == ILL_COMPOSITE else TOL_COMPOSITE), (name, e)


def test_a_failed_path_keeps_its_times_and_gets_finite_zero_gradients(gpu_ctx):
    batch = pr.random_batch(3, 4, seed0=65000)
    times_np = util.oracle_times(batch)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        times = _dev(times_np)
        coeffs = _solve(plan, batch, times)
        coeffs[4:8] = float("nan")                     # path 1: what a failed solve may leave behind
        status = torch.tensor([1, -2, 1], dtype=torch.int32, device="cuda")
        c = coeffs.clone().requires_grad_(True)
        t = times.clone().requires_grad_(True)
        lim = _dev(np.tile(pr.DEFAULT_LIMITS * 0.3, (1, 1))).expand(3, 9).clone().requires_grad_(True)
        r = _dev(np.random.default_rng(2).standard_normal(12))
        t1 = autograd.scale_times_to_limits(plan, c, t, lim, status)
        (t1 * r).sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert torch.equal(t1[4:8].detach(), times[4:8])
    assert torch.all(torch.isfinite(c.grad)) and torch.all(torch.isfinite(t.grad)) and torch.all(torch.isfinite(lim.grad))
    assert torch.all(c.grad[4:8] == 0.0) and torch.all(lim.grad[1] == 0.0) and torch.equal(t.grad[4:8], r[4:8])
    assert torch.any(t1[:4].detach() != times[:4]) and torch.any(lim.grad[0] != 0.0)

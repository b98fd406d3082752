"""mrs_tg_plan_sample_states_vjp on the GPU (sample_vjp_kernel), mrs_tg_plan_sample, and the
autograd Functions on top of them: the 60-digit fixtures and the CPU harness, the walk against the forward sampler, torch
autograd of a gathered Horner restatement, gradcheck, the chain solve -> sample, determinism, degenerate paths, overflow."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from tests import sample_vjp_util as su
from tests import util

pytestmark = pytest.mark.gpu

TOL_WELL, TOL_ILL, ILL_CASE = 1e-10, 1e-5, "ratio50"   # the CPU tier's bounds (test_vjp_host.py, test_gpu_vjp.py)
TOL_GPU_CPU = 1e-13
NAN = float("nan")


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _vjp(plan, coeffs, times, dt, cap, G=None, status=None, want=("gc", "gt", "seg", "time", "n")):
    """every wanted output NaN / -1 prefilled -> dict of host arrays"""
    P, nS = plan.n_paths, plan.n_segments
    o = dict(gc=torch.full((nS, 4, 10), NAN, dtype=torch.float64, device="cuda") if "gc" in want else None,
             gt=torch.full((nS,), NAN, dtype=torch.float64, device="cuda") if "gt" in want else None,
             seg=torch.full((P, cap), -1, dtype=torch.int32, device="cuda") if "seg" in want else None,
             time=torch.full((P, cap), NAN, dtype=torch.float64, device="cuda") if "time" in want else None,
             n=torch.full((P,), -1, dtype=torch.int32, device="cuda") if "n" in want else None)
    plan.sample_states_vjp(coeffs, times, dt, cap, G, status=status, grad_coeffs=o["gc"], grad_seg_times=o["gt"],
                           sample_segment=o["seg"], sample_time=o["time"], n_samples=o["n"])
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _gather(so, seg, n, cap):
    """flat sample list of a batch: (path, index in path, global segment row, first segment row of the path)"""
    rows = np.minimum(n, cap)
    p_idx = np.repeat(np.arange(len(rows)), rows)
    k_idx = np.concatenate([np.arange(r) for r in rows]) if len(rows) else np.zeros(0, dtype=np.int64)
    first = np.asarray(so[:-1], dtype=np.int64)[p_idx]
    return p_idx, k_idx, first + seg[p_idx, k_idx].astype(np.int64), first


def _torch_gradients(so, coeffs, times, seg, n, dt, cap, G):
    """torch autograd of L = sum G . states of the gathered Horner expression over the first min(n, cap) samples"""
    p_idx, k_idx, gseg, first = _gather(so, seg, n, cap)
    c = coeffs.detach().clone().requires_grad_(True)
    T = times.detach().clone().requires_grad_(True)
    Gf = G.reshape(G.shape[0], cap, -1, 4)
    no = Gf.shape[2]
    tk = su.sample_times_expr(torch, T, so, _dev(p_idx), _dev(gseg - first), _dev(k_idx), dt)
    st = su.states_at(torch, c, _dev(gseg), tk, no)
    (st * Gf[_dev(p_idx), _dev(k_idx)]).sum().backward()
    torch.cuda.synchronize()
    return c.grad.cpu().numpy(), T.grad.cpu().numpy()


def _path_errors(so, gc, gt, rc, rt):
    """per path: largest |difference| over its coefficient and time gradients, relative to its largest reference entry"""
    so = np.asarray(so, dtype=np.int64)
    diff = np.maximum(np.max(np.abs(gc - rc).reshape(len(gt), -1), axis=1), np.abs(gt - rt))
    mag = np.maximum(np.max(np.abs(rc).reshape(len(rt), -1), axis=1), np.abs(rt))
    return np.maximum.reduceat(diff, so[:-1]) / np.maximum(np.maximum.reduceat(mag, so[:-1]), 1e-300)


def test_the_library_reports_the_capability(gpu_ctx):
    assert api.CAP_SAMPLE_GRADIENT == 32 and api.KERNEL_SAMPLE_VJP == 5
    assert api.capabilities() & api.CAP_SAMPLE_GRADIENT
    batch = pr.random_batch(8, 4, seed0=60000)
    out = gpu_ctx.solve_batch(batch, None)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        gpu_ctx.set_profiling(True)
        _vjp(plan, _dev(out["coeffs"]), _dev(out["times"]), 0.2, 256, _dev(np.ones((8, 256, 4))))
        assert gpu_ctx.last_kernel_ms(api.KERNEL_SAMPLE_VJP) > 0
    finally:
        gpu_ctx.set_profiling(False)
        plan.close()


def test_fixtures_through_the_abi_and_the_cpu_harness(gpu_ctx, tmp_path):
    cases = su.load_cases()
    exe = su.build_harness(tmp_path)
    cpu = su.run_harness(exe, [su.case_problem(c) for c in cases])
    rows = []
    for case, h in zip(cases, cpu):
        S, cap, no = len(case["seg_times"]), case["capacity"], case["n_orders"]
        G = np.full((1, cap, no, 4), np.nan)   # rows at or beyond the sample count hold NaN: never read
        g = np.asarray(case["grad_states"], dtype=np.float64).reshape(-1, no, 4)
        G[0, :g.shape[0]] = g
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            o = _vjp(plan, _dev(case["coeffs"]), _dev(case["seg_times"]), case["dt"], cap, _dev(G if no == 5 else G[:, :, 0]))
        finally:
            plan.close()
        rows_n = min(case["n_samples"], cap)
        assert o["n"][0] == case["n_samples"] == h["n"], case["name"]
        assert np.array_equal(o["seg"][0, :rows_n], np.array(case["sample_segment"])), case["name"]
        assert np.array_equal(o["time"][0, :rows_n], h["sample_time"]), case["name"]   # the same additions in the same order
        assert np.all(o["seg"][0, rows_n:] == -1) and np.all(np.isnan(o["time"][0, rows_n:])), case["name"]
        assert np.all(np.isfinite(o["gc"])) and np.all(np.isfinite(o["gt"])), case["name"]
        e = su.fixture_error(case, o["gc"], o["gt"])
        scale = max(np.max(np.abs(h["grad_coeffs"])), np.max(np.abs(h["grad_seg_times"])))
        vs_cpu = max(np.max(np.abs(o["gc"] - h["grad_coeffs"])), np.max(np.abs(o["gt"] - h["grad_seg_times"]))) / scale
        same_bits = np.array_equal(o["gc"], h["grad_coeffs"]) and np.array_equal(o["gt"], h["grad_seg_times"])
        rows.append((case["name"], e, vs_cpu, same_bits))
        print("SAMPLE VJP GPU FIXTURE %s: vs 60 digits %.1e, vs CPU harness %.1e, bit-identical %s" % rows[-1])
        assert e <= TOL_WELL, rows[-1]
        assert vs_cpu <= TOL_GPU_CPU, rows[-1]


@pytest.mark.parametrize("n_seg,dt", [(10, 0.2), ("ragged", 0.2), (6, 0.05)])
def test_the_walk_is_the_forward_samplers(gpu_ctx, n_seg, dt):
    batch = pr.random_batch(48, n_seg, seed0=77)
    cap = 4096
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, sampling_dt=dt, sample_capacity=cap)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        coeffs, times = _dev(out["coeffs"]), _dev(out["times"])
        n_fwd = torch.zeros(batch.n_paths, dtype=torch.int32, device="cuda")
        states = torch.full((batch.n_paths, cap, api.STATE_ORDERS, 4), NAN, dtype=torch.float64, device="cuda")
        plan.sample_states(coeffs, times, dt, cap, n_fwd, states)
        o = _vjp(plan, coeffs, times, dt, cap, want=("seg", "time", "n"))
    finally:
        plan.close()
    n = n_fwd.cpu().numpy()
    assert np.array_equal(o["n"], n) and np.all(n > 0)
    beyond = np.arange(cap)[None, :] >= n[:, None]
    assert np.all(o["seg"][beyond] == -1) and np.all(np.isnan(o["time"][beyond]))   # untouched beyond the count
    p_idx, k_idx, gseg, _ = _gather(batch.seg_offsets, o["seg"], n, cap)
    st = su.states_at(torch, coeffs, _dev(gseg), _dev(o["time"][p_idx, k_idx])).cpu().numpy()
    fwd = states.cpu().numpy()[p_idx, k_idx]
    for k in range(api.STATE_ORDERS):
        scale = max(1.0, float(np.max(np.abs(fwd[:, k]))))
        d = np.abs(st[:, k] - fwd[:, k])
        if k == 0:   # the forward's heading is wrapped
            d[:, 3] = np.abs(np.remainder(d[:, 3] + np.pi, 2 * np.pi) - np.pi)
        assert np.max(d) < 1e-11 * scale, (k, np.max(d))


def test_plan_sample_is_order_0_of_the_states_and_the_solves_own_samples(gpu_ctx):
    batch = pr.random_batch(48, "ragged", seed0=78)
    dt, cap = 0.2, 1024
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, sampling_dt=dt, sample_capacity=cap)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        coeffs, times = _dev(out["coeffs"]), _dev(out["times"])
        n_a = torch.zeros(batch.n_paths, dtype=torch.int32, device="cuda")
        n_b = torch.zeros_like(n_a)
        states = torch.full((batch.n_paths, cap, api.STATE_ORDERS, 4), NAN, dtype=torch.float64, device="cuda")
        samples = torch.full((batch.n_paths, cap, 4), NAN, dtype=torch.float64, device="cuda")
        plan.sample_states(coeffs, times, dt, cap, n_a, states)
        plan.sample(coeffs, times, dt, cap, n_b, samples)
        torch.cuda.synchronize()
        assert torch.equal(n_a, n_b) and np.array_equal(n_b.cpu().numpy(), out["n_samples"])
        assert np.array_equal(samples.cpu().numpy(), states[:, :, 0].cpu().numpy(), equal_nan=True)
        for p in range(batch.n_paths):
            r = min(int(out["n_samples"][p]), cap)
            assert np.array_equal(samples[p, :r].cpu().numpy(), out["samples"][p, :r])
        # the autograd Functions' forwards: the same bits, zero rows beyond the count
        s2, n2 = autograd.sample(plan, coeffs, times, dt, cap)
        st2, n3 = autograd.sample_states(plan, coeffs, times, dt, cap)
        torch.cuda.synchronize()
        assert torch.equal(n2, n_a) and torch.equal(n3, n_a)
        assert torch.equal(s2, torch.nan_to_num(samples, nan=0.0)) and torch.equal(st2, torch.nan_to_num(states, nan=0.0))
        assert not s2.requires_grad and not n2.requires_grad
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()


def _check_against_torch(gpu_ctx, batch, coeffs_h, times_h, dt, cap, no, seed, label):
    rng = np.random.default_rng(seed)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        coeffs, times = _dev(coeffs_h), _dev(times_h)
        shape = (batch.n_paths, cap, 5, 4) if no == 5 else (batch.n_paths, cap, 4)
        G = _dev(rng.standard_normal(shape))
        o = _vjp(plan, coeffs, times, dt, cap, G)
    finally:
        plan.close()
    rc, rt = _torch_gradients(batch.seg_offsets, coeffs, times, o["seg"], o["n"], dt, cap, G)
    assert np.all(np.isfinite(o["gc"])) and np.all(np.isfinite(o["gt"]))
    errs = _path_errors(batch.seg_offsets, o["gc"], o["gt"], rc, rt)
    print("SAMPLE VJP GPU vs TORCH %s n_orders=%d: %d paths, max %.2e, median %.2e, overflowing %d" %
          (label, no, errs.size, errs.max(), np.median(errs), int(np.sum(o["n"] > cap))))
    return errs, o


@pytest.mark.parametrize("no", [1, 5])
def test_1024x10_against_torch_autograd_of_the_gathered_horner(gpu_ctx, no):
    batch = pr.random_batch(1024, 10, seed0=61000)
    out = gpu_ctx.solve_batch(batch, None)
    errs, o = _check_against_torch(gpu_ctx, batch, out["coeffs"], out["times"], 0.2, 640, no, 5 + no, "1024x10")
    assert errs.max() <= TOL_WELL


@pytest.mark.parametrize("no", [1, 5])
def test_mixed_ragged_8192_against_torch_autograd_of_the_gathered_horner(gpu_ctx, no):
    batch = pr.random_mixed_batch(8192, seed0=62000)
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER)   # (uneven times)
    ok = out["status"] > 0
    assert ok.mean() > 0.9
    cap = 768
    errs, o = _check_against_torch(gpu_ctx, batch, np.nan_to_num(out["coeffs"]), out["times"], 0.2, cap, no, 9 + no, "mixed 8192")
    good = ok & np.isfinite(errs)
    assert np.all(np.isfinite(errs[ok]))
    assert errs[good].max() <= TOL_WELL


def test_overflowing_paths_use_the_first_capacity_samples(gpu_ctx):
    batch = pr.random_batch(64, "ragged", seed0=63000)
    out = gpu_ctx.solve_batch(batch, None)
    n_all = np.array([int(np.sum(out["times"][a:b]) / 0.2) for a, b in zip(batch.seg_offsets[:-1], batch.seg_offsets[1:])])
    cap = int(np.median(n_all))
    for no in (1, 5):
        errs, o = _check_against_torch(gpu_ctx, batch, out["coeffs"], out["times"], 0.2, cap, no, 20 + no, "overflow")
        assert np.any(o["n"] == cap + 1) and np.any(o["n"] <= cap) and np.all(o["n"] <= cap + 1)
        assert errs.max() <= TOL_WELL


def _nudged_times(t, so, dt, margin):
    """times moved so that every sample k >= 1 lies at least `margin` from both ends of its segment and the last sample at
    least `margin` before the end (the condition under which a finite difference of the samples means something)"""
    t = np.array(t, dtype=np.float64)
    for a, b in zip(so[:-1], so[1:]):
        cum = 0.0
        for i in range(a, b):
            while True:
                f = np.fmod(cum + t[i], dt)
                if min(f, dt - f) >= 2 * margin:
                    break
                t[i] += 0.25 * dt
            cum += t[i]
    return t


def _assert_margin(t, so, dt, margin):
    for a, b in zip(so[:-1], so[1:]):
        f = np.fmod(np.cumsum(t[a:b]), dt)
        assert np.all(np.minimum(f, dt - f) >= margin)


def test_gradcheck_of_the_autograd_functions(gpu_ctx):
    """Finite differences mean something where no sample changes its segment and no heading crosses the seam under the
    perturbation: segment times of 1 .. 1.3 s (d sample / d c_9 = t^9 stays below 11, so a coefficient step of 1e-5 moves a
    heading by 1e-4 at most), nudged to a margin of 1e-3 s, and every sampled heading at least 1e-2 from +-pi (asserted)."""
    batch = pr.random_batch(4, 4, seed0=64000)
    dt, margin = 0.2, 1e-3
    t = _nudged_times(1.0 + 0.3 * np.random.default_rng(3).random(batch.n_segments), batch.seg_offsets, dt, margin)
    _assert_margin(t, batch.seg_offsets, dt, margin)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask, fv0 = _dev(batch.fixed_mask), _dev(batch.fixed_values)
    times0 = _dev(t)
    try:
        coeffs0, _, status = autograd.solve(plan, mask, fv0, times0)
        cap = int(max(np.sum(t[a:b]) / dt for a, b in zip(batch.seg_offsets[:-1], batch.seg_offsets[1:]))) + 4
        s0, n0 = autograd.sample(plan, coeffs0, times0, dt, cap, status)
        torch.cuda.synchronize()
        assert bool(torch.all(status > 0)) and bool(torch.all(n0 <= cap)) and bool(torch.all(n0 > 8))
        assert float(s0[..., 3].abs().max()) < np.pi - 1e-2
        coeffs = coeffs0.detach().clone().requires_grad_(True)
        times = times0.clone().requires_grad_(True)
        # (eps 1e-5: far inside the margins; the samples are exactly linear in the coefficients and smooth in the times)
        assert torch.autograd.gradcheck(lambda c, tt: autograd.sample(plan, c, tt, dt, cap)[0], (coeffs, times),
                                        eps=1e-5, atol=1e-5, rtol=1e-3)
        assert torch.autograd.gradcheck(lambda c, tt: autograd.sample_states(plan, c, tt, dt, cap)[0], (coeffs, times),
                                        eps=1e-5, atol=1e-5, rtol=1e-3)
        fv = fv0.clone().requires_grad_(True)

        def chain(v, tt):
            c, _, st = autograd.solve(plan, mask, v, tt)
            return autograd.sample(plan, c, tt, dt, cap, st)[0]
        assert torch.autograd.gradcheck(chain, (fv, times), eps=1e-5, atol=1e-5, rtol=1e-3)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()


def test_composite_fixtures_through_solve_and_sample(gpu_ctx):
    for case in su.load_composite_cases():
        S, cap, d = len(case["seg_times"]), case["capacity"], case["derivative_to_optimize"]
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            fv = _dev(np.array(case["fixed_values"], dtype=np.float64)).requires_grad_(True)
            times = _dev(case["seg_times"]).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, _dev(np.array(case["fixed_mask"]), np.uint8), fv, times, derivative=d)
            samples, n = autograd.sample(plan, coeffs, times, case["dt"], cap, status)
            G = torch.zeros_like(samples)
            G[0, :case["n_samples"]] = _dev(np.array(case["grad_samples"]))
            (samples * G).sum().backward()
            torch.cuda.synchronize()
            gpu_ctx.use_torch_stream()
        finally:
            plan.close()
        assert int(n[0]) == case["n_samples"] and int(status[0]) > 0
        rv, rt = np.array(case["grad_fixed_values"]), np.array(case["grad_seg_times"])
        scale = max(np.max(np.abs(rv)), np.max(np.abs(rt)))
        e = max(np.max(np.abs(fv.grad.cpu().numpy() - rv)), np.max(np.abs(times.grad.cpu().numpy() - rt))) / scale
        print("SAMPLE VJP GPU COMPOSITE %s: %.1e" % (case["name"], e))
        assert e <= (TOL_ILL if case["name"] == ILL_CASE else TOL_WELL), (case["name"], e)


def _loss_grads(plan, c0, t0, G, dt, cap, states, stream=None):
    c = c0.clone().requires_grad_(True)
    tt = t0.clone().requires_grad_(True)
    s = stream if stream is not None else torch.cuda.default_stream()
    s.wait_stream(torch.cuda.default_stream())
    with torch.cuda.stream(s):
        out, n = (autograd.sample_states if states else autograd.sample)(plan, c, tt, dt, cap)
        (out * G).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), c.grad.cpu().numpy(), tt.grad.cpu().numpy()


def test_streams_and_repeats_give_the_same_bits(gpu_ctx):
    batch = pr.random_batch(1024, 10, seed0=65000)
    out = gpu_ctx.solve_batch(batch, None)
    dt, cap = 0.2, 640
    c, t = _dev(out["coeffs"]), _dev(out["times"])
    rng = np.random.default_rng(12)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        for states in (False, True):
            G = _dev(rng.standard_normal((1024, cap, 5, 4) if states else (1024, cap, 4)))
            a = _loss_grads(plan, c, t, G, dt, cap, states)
            b = _loss_grads(plan, c, t, G, dt, cap, states)
            z = _loss_grads(plan, c, t, G, dt, cap, states, stream=torch.cuda.Stream())
            for x, y, w in zip(a, b, z):
                assert np.array_equal(x, y) and np.array_equal(x, w)
            assert np.all(np.isfinite(a[1])) and np.any(a[2] != 0.0)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()


def test_degenerate_paths_and_arguments(gpu_ctx):
    batch = pr.random_batch(6, 5, seed0=66000)
    out = gpu_ctx.solve_batch(batch, None)
    dt, cap = 0.2, 512
    rng = np.random.default_rng(13)
    Gh = rng.standard_normal((6, cap, 5, 4))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t = _dev(out["coeffs"]), _dev(out["times"])
        ref = _vjp(plan, c, t, dt, cap, _dev(Gh))
        n = ref["n"]
        # NaN upstream rows at or beyond the count change nothing
        Gn = Gh.copy()
        for p in range(6):
            Gn[p, n[p]:] = np.nan
        o = _vjp(plan, c, t, dt, cap, _dev(Gn))
        assert np.array_equal(o["gc"], ref["gc"]) and np.array_equal(o["gt"], ref["gt"])
        # status <= 0 with NaN coefficients: zero rows, the other paths' bits untouched
        ch = out["coeffs"].copy()
        ch[5:10] = np.nan
        status = np.ones(6, dtype=np.int32)
        status[1] = -2
        o = _vjp(plan, _dev(ch), t, dt, cap, _dev(Gh), status=_dev(status))
        assert np.all(o["gc"][5:10] == 0.0) and np.all(o["gt"][5:10] == 0.0)
        keep = np.r_[0:5, 10:30]
        assert np.array_equal(o["gc"][keep], ref["gc"][keep]) and np.array_equal(o["gt"][keep], ref["gt"][keep])
        assert np.array_equal(o["n"], n)
        # NaN times: no samples, zero rows
        th = out["times"].copy()
        th[12] = np.nan
        o = _vjp(plan, c, _dev(th), dt, cap, _dev(Gh))
        assert o["n"][2] == 0 and np.all(o["gc"][10:15] == 0.0) and np.all(o["gt"][10:15] == 0.0)
        assert np.all(o["seg"][2] == -1)
        keep = np.r_[0:10, 15:30]
        assert np.array_equal(o["gc"][keep], ref["gc"][keep]) and np.array_equal(o["gt"][keep], ref["gt"][keep])
        # capacity 0 with the counts only
        o = _vjp(plan, c, t, dt, 0, want=("n",))
        assert np.all(o["n"] == 1)
        # invalid calls
        G = _dev(Gh)
        gc = torch.zeros((30, 4, 10), dtype=torch.float64, device="cuda")
        n_dev = torch.zeros(6, dtype=torch.int32, device="cuda")
        with pytest.raises(api.MrsTgError):   # no output
            plan.sample_states_vjp(c, t, dt, cap, G)
        with pytest.raises(api.MrsTgError):   # a gradient without the upstream
            plan.sample_states_vjp(c, t, dt, cap, None, grad_coeffs=gc)
        with pytest.raises(api.MrsTgError):   # n_orders 3
            plan.sample_states_vjp(c, t, dt, cap, G[:, :, :3].contiguous(), grad_coeffs=gc)
        with pytest.raises(api.MrsTgError):   # no coefficients
            plan.sample_states_vjp(None, t, dt, cap, G, grad_coeffs=gc)
        with pytest.raises(api.MrsTgError):   # dt = 0
            plan.sample_states_vjp(c, t, 0.0, cap, None, n_samples=n_dev)
        with pytest.raises(api.MrsTgError):
            plan.sample(c, t, dt, 16, n_dev, None)
    finally:
        plan.close()

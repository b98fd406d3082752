"""mrs_tg_plan_evaluate / mrs_tg_plan_evaluate_vjp on the GPU (evaluate_kernel, evaluate_vjp_kernel) and
autograd.evaluate on top of them: the 60-digit fixtures and the CPU harness, the sampler as a special case, torch autograd of
a gathered Horner restatement, gradcheck, the chain solve -> evaluate, query order, determinism, degenerate paths and
arguments, long paths and many queries.  NaN inputs are ordinary data here: nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from tests import evaluate_util as eu

pytestmark = pytest.mark.gpu

TOL_WELL, TOL_ILL, ILL_CASE = 1e-10, 1e-5, "ratio50"   # the CPU tier's bounds (test_vjp_host.py, test_sample_vjp_host.py)
TOL_GPU_CPU = 1e-13
ERR_INVALID_ARG = -1   # MRS_TG_ERR_INVALID_ARG (include/mrs_tg.h)
NAN = float("nan")
EPS = 2.0 ** -52


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _eval(plan, coeffs, times, q, no):
    """states, segment, local time as host arrays; every output prefilled with NaN / -7"""
    P, Q = q.shape
    st = torch.full((P, Q, no, 4), NAN, dtype=torch.float64, device="cuda")
    seg = torch.full((P, Q), -7, dtype=torch.int32, device="cuda")
    tau = torch.full((P, Q), NAN, dtype=torch.float64, device="cuda")
    plan.evaluate(coeffs, times, q, st, query_segment=seg, query_local_time=tau)
    torch.cuda.synchronize()
    return st.cpu().numpy(), seg.cpu().numpy(), tau.cpu().numpy()


def _vjp(plan, coeffs, times, q, G, status=None, want=("gc", "gt", "gq")):
    """every wanted output NaN prefilled -> dict of host arrays"""
    o = dict(gc=torch.full((plan.n_segments, 4, 10), NAN, dtype=torch.float64, device="cuda") if "gc" in want else None,
             gt=torch.full((plan.n_segments,), NAN, dtype=torch.float64, device="cuda") if "gt" in want else None,
             gq=torch.full(tuple(q.shape), NAN, dtype=torch.float64, device="cuda") if "gq" in want else None)
    plan.evaluate_vjp(coeffs, times, q, G, status=status, grad_coeffs=o["gc"], grad_seg_times=o["gt"], grad_query_times=o["gq"])
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _rel(a, b, scale):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / scale) if np.asarray(a).size else 0.0


def test_the_library_reports_the_capability_and_times_both_kernels(gpu_ctx):
    assert api.CAP_EVALUATE == 64 and api.KERNEL_EVALUATE == 6 and api.KERNEL_EVALUATE_VJP == 7
    assert api.capabilities() & api.CAP_EVALUATE
    batch = pr.random_batch(8, 4, seed0=70000)
    out = gpu_ctx.solve_batch(batch, None)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        gpu_ctx.set_profiling(True)
        q = _dev(np.tile(np.linspace(0.0, 2.0, 33), (8, 1)))
        c, t = _dev(out["coeffs"]), _dev(out["times"])
        _eval(plan, c, t, q, 5)
        _vjp(plan, c, t, q, _dev(np.ones((8, 33, 5, 4))))
        assert gpu_ctx.last_kernel_ms(api.KERNEL_EVALUATE) > 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_EVALUATE_VJP) > 0
    finally:
        gpu_ctx.set_profiling(False)
        plan.close()


def test_fixtures_through_the_abi_and_the_cpu_harness(gpu_ctx, tmp_path):
    cases = eu.load_cases()
    exe = eu.build_harness(tmp_path)
    cpu = eu.run_harness(exe, [eu.case_problem(c) for c in cases])
    for case, h in zip(cases, cpu):
        S, no = len(case["seg_times"]), case["n_orders"]
        q = _dev(eu.query_array(case)[None, :])
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            c, t = _dev(case["coeffs"]), _dev(case["seg_times"])
            st, seg, tau = _eval(plan, c, t, q, no)
            assert np.array_equal(seg[0], np.array(case["query_segment"])), case["name"]
            assert np.array_equal(seg[0], h["query_segment"]) and np.array_equal(tau[0], h["query_local_time"]), case["name"]
            scale = max(np.max(np.abs(h["states"])), 1e-300)
            vs_cpu = _rel(st[0], h["states"], scale)
            bits = np.array_equal(st[0], h["states"])
            assert vs_cpu <= TOL_GPU_CPU, (case["name"], vs_cpu)
            if case.get("forward"):
                worst, ok = eu.forward_error(case, st[0])
                print("EVALUATE GPU FORWARD FIXTURE %s: vs 60 digits %.1e, vs CPU harness %.1e, bit-identical %s" %
                      (case["name"], worst, vs_cpu, bits))
                assert ok, (case["name"], worst)
                assert np.all(st[0][seg[0] < 0] == 0.0) and np.all(tau[0][seg[0] < 0] == 0.0)
                continue
            o = _vjp(plan, c, t, q, _dev(np.array(case["grad_states"])[None]))
        finally:
            plan.close()
        for k in ("gc", "gt", "gq"):
            assert np.all(np.isfinite(o[k])), (case["name"], k)
        e = eu.fixture_error(case, o["gc"], o["gt"], o["gq"][0])
        gscale = max(np.max(np.abs(h["grad_coeffs"])), np.max(np.abs(h["grad_seg_times"])), np.max(np.abs(h["grad_query_times"])))
        g_cpu = max(_rel(o["gc"], h["grad_coeffs"], gscale), _rel(o["gt"], h["grad_seg_times"], gscale),
                    _rel(o["gq"][0], h["grad_query_times"], gscale))
        gbits = (np.array_equal(o["gc"], h["grad_coeffs"]) and np.array_equal(o["gt"], h["grad_seg_times"]) and
                 np.array_equal(o["gq"][0], h["grad_query_times"]))
        print("EVALUATE GPU FIXTURE %s: vs 60 digits %.1e, vs CPU harness %.1e (states %.1e), bit-identical %s (states %s)" %
              (case["name"], e, g_cpu, vs_cpu, gbits, bits))
        assert e <= TOL_WELL, (case["name"], e)
        assert g_cpu <= TOL_GPU_CPU, (case["name"], g_cpu)


def _repeated_additions(dt, count):
    A = np.zeros(count, dtype=np.float64)
    acc = 0.0
    for k in range(1, count):
        acc = acc + dt
        A[k] = acc
    return A


@pytest.mark.parametrize("n_seg,paths,dt", [(10, 1024, 0.2), ("ragged", 512, 0.2), (6, 512, 0.05)])
def test_the_sampler_is_a_special_case(gpu_ctx, n_seg, paths, dt):
    """Path p asked at A[k], the k-fold repeated addition of dt, k < n_p (NaN beyond): the segment of EVERY sample is the
    walk's and every state within 2 |dtau| |p^(o+1)(tau)| + the Horner rounding bound of the sampler's.  The samples of the
    first segment have tau == A[k] in both routes: their order 0 (positions and heading, what mrs_tg_plan_sample and the
    solve calls write) is the sampler's bits.  Their orders 1..4 are held to the bound as well and not to bit equality:
    sample_kernel<4> leaves the fusion of acc * t + ff * c to the compiler, which rounds ff * c in the first step of a chain
    and acc * t in the later ones (DESIGN.md section 7c names the instructions); the shared routine fixes one of the two."""
    batch = pr.random_batch(paths, n_seg, seed0=77)
    out = gpu_ctx.solve_batch(batch, None)   # the library's estimator, then the fixed-times solve
    assert np.all(out["status"] > 0)
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    totals = np.add.reduceat(out["times"], so[:-1])
    cap = int(np.max(totals) / dt) + 8
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t = _dev(out["coeffs"]), _dev(out["times"])
        n_dev = torch.zeros(paths, dtype=torch.int32, device="cuda")
        walk_seg = torch.full((paths, cap), -1, dtype=torch.int32, device="cuda")
        walk_tau = torch.full((paths, cap), NAN, dtype=torch.float64, device="cuda")
        sampled = torch.zeros((paths, cap, 5, 4), dtype=torch.float64, device="cuda")
        plan.sample_states(c, t, dt, cap, n_dev, sampled)
        plan.sample_states_vjp(c, t, dt, cap, None, sample_segment=walk_seg, sample_time=walk_tau)
        torch.cuda.synchronize()
        n = n_dev.cpu().numpy()
        assert np.all(n > 0) and np.all(n <= cap)
        has = np.arange(cap)[None, :] < n[:, None]
        q = np.where(has, _repeated_additions(dt, cap)[None, :], np.nan)
        st, seg, tau = _eval(plan, c, t, _dev(q), 5)
    finally:
        plan.close()
    ws, wt, sm = walk_seg.cpu().numpy(), walk_tau.cpu().numpy(), sampled.cpu().numpy()
    wrong = int(np.sum(seg[has] != ws[has]))
    dtau = np.abs(tau[has] - wt[has])
    print("EVALUATE GPU vs SAMPLER %s x %s dt %.2f: %d samples, %d segment disagreements, max |dtau| %.2e" %
          (paths, n_seg, dt, int(has.sum()), wrong, float(dtau.max())))
    assert wrong == 0
    assert np.all(seg[~has] == -1) and np.all(st[~has] == 0.0)
    p_idx, k_idx = np.nonzero(has)
    gseg = _dev(so[p_idx] + seg[p_idx, k_idx])
    tmax = _dev(np.maximum(np.abs(tau[has]), np.abs(wt[has])))
    cd = c.reshape(-1, 4, 10)
    a, b = st[has], sm[has]
    worst = 0.0
    for o in range(5):
        slope = eu.derivative_at(torch, cd, gseg, _dev(tau[has]), o + 1).abs().cpu().numpy()
        horner = eu.derivative_at(torch, cd, gseg, tmax, o, absolute=True).cpu().numpy() * 64 * EPS
        bound = 2.0 * dtau[:, None] * slope + horner
        d = np.abs(a[:, o] - b[:, o])
        if o == 0:   # the heading modulo 2 pi
            d[:, 3] = np.abs(np.remainder(d[:, 3] + np.pi, 2 * np.pi) - np.pi)
        assert np.all(d <= bound), (o, float(np.max(d - bound)))
        worst = max(worst, float(np.max(d / np.maximum(bound, 1e-300))))
    first = seg[has] == 0
    same0 = np.array_equal(a[first][:, 0], b[first][:, 0])
    print("EVALUATE GPU vs SAMPLER: worst difference / bound %.2f; first-segment samples: %d, order 0 bit-identical %s, orders "
          "1..4 bit-identical %s; all samples: order 0 bit-identical %s" %
          (worst, int(first.sum()), same0, np.array_equal(a[first][:, 1:], b[first][:, 1:]), np.array_equal(a[:, 0], b[:, 0])))
    assert np.array_equal(tau[has][first], q[has][first])
    assert first.sum() > paths and same0


def _random_queries(rng, so, times, Q):
    """[P][Q] unsorted query times: most inside the path, some behind its end, some negative, some NaN, some on a vertex"""
    totals = np.add.reduceat(times, np.asarray(so[:-1], dtype=np.int64))
    q = rng.uniform(0.0, 1.0, size=(len(totals), Q)) * totals[:, None]
    kind = rng.integers(0, 20, size=q.shape)
    q[kind == 0] = np.nan
    q[kind == 1] *= -1.0
    q[kind == 2] += totals[:, None].repeat(Q, axis=1)[kind == 2] + 0.5
    q[:, 0] = 0.0
    q[:, 1] = totals
    return q


def _torch_gradients(so, coeffs, times, q, seg, G):
    """torch autograd of L = sum G . states of the gathered Horner expression at the kernel's own segments"""
    inr = seg >= 0
    p_idx, k_idx = np.nonzero(inr)
    first = np.asarray(so[:-1], dtype=np.int64)[p_idx]
    c = coeffs.detach().clone().requires_grad_(True)
    T = times.detach().clone().requires_grad_(True)
    qq = q.detach().clone().requires_grad_(True)
    seg_rel = _dev(seg[p_idx, k_idx].astype(np.int64))
    tau = eu.local_time_expr(torch, T, so, _dev(p_idx), seg_rel, qq[_dev(p_idx), _dev(k_idx)])
    st = eu.states_at(torch, c, _dev(first) + seg_rel, tau, G.shape[2])
    (st * G[_dev(p_idx), _dev(k_idx)]).sum().backward()
    torch.cuda.synchronize()
    return c.grad.cpu().numpy(), T.grad.cpu().numpy(), torch.nan_to_num(qq.grad, nan=0.0).cpu().numpy(), tau.detach().cpu().numpy()


def _path_errors(so, o, rc, rt, rq):
    """per path: largest |difference| over its three gradients, relative to its largest reference entry"""
    so = np.asarray(so, dtype=np.int64)
    diff = np.maximum(np.max(np.abs(o["gc"] - rc).reshape(len(rt), -1), axis=1), np.abs(o["gt"] - rt))
    mag = np.maximum(np.max(np.abs(rc).reshape(len(rt), -1), axis=1), np.abs(rt))
    diff = np.maximum(np.maximum.reduceat(diff, so[:-1]), np.max(np.abs(o["gq"] - rq), axis=1))
    mag = np.maximum(np.maximum.reduceat(mag, so[:-1]), np.max(np.abs(rq), axis=1))
    return diff / np.maximum(mag, 1e-300)


def _check_against_torch(gpu_ctx, batch, coeffs_h, times_h, Q, no, seed, label, status=None):
    rng = np.random.default_rng(seed)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t = _dev(coeffs_h), _dev(times_h)
        q = _dev(_random_queries(rng, batch.seg_offsets, times_h, Q))
        G = _dev(rng.standard_normal((batch.n_paths, Q, no, 4)))
        st, seg, tau = _eval(plan, c, t, q, no)
        G[_dev(seg < 0)] = NAN   # (the upstream row of an out-of-range query is never read)
        o = _vjp(plan, c, t, q, G, status=status)
    finally:
        plan.close()
    rc, rt, rq, rtau = _torch_gradients(batch.seg_offsets, c, t, q, seg, G)
    # (both routes sum at most 30 segment times in front of a query: each within 32 eps of the path's total time)
    totals = np.add.reduceat(np.abs(times_h), np.asarray(batch.seg_offsets[:-1], dtype=np.int64))
    assert np.all(np.abs(rtau - tau[seg >= 0]) <= 64 * EPS * totals[np.nonzero(seg >= 0)[0]])
    errs = _path_errors(batch.seg_offsets, o, rc, rt, rq)
    print("EVALUATE VJP GPU vs TORCH %s n_orders=%d: %d paths, %d of %d queries in range, max %.2e, median %.2e" %
          (label, no, errs.size, int(np.sum(seg >= 0)), seg.size, np.nanmax(errs), np.nanmedian(errs)))
    return errs, o, seg


@pytest.mark.parametrize("no", [1, 5])
def test_1024x10_against_torch_autograd_of_the_gathered_horner(gpu_ctx, no):
    batch = pr.random_batch(1024, 10, seed0=71000)
    out = gpu_ctx.solve_batch(batch, None)
    errs, o, seg = _check_against_torch(gpu_ctx, batch, out["coeffs"], out["times"], 150, no, 5 + no, "1024x10")
    for k in ("gc", "gt", "gq"):
        assert np.all(np.isfinite(o[k])), k
    assert np.all(o["gq"][seg < 0] == 0.0)
    assert errs.max() <= TOL_WELL   # (the sampler's bound for the same comparison, test_gpu_sample_vjp.py)


@pytest.mark.parametrize("no", [1, 5])
def test_mixed_ragged_8192_against_torch_autograd_of_the_gathered_horner(gpu_ctx, no):
    batch = pr.random_mixed_batch(8192, seed0=72000)
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER)   # (uneven times)
    ok = out["status"] > 0
    assert ok.mean() > 0.9
    status = _dev(out["status"], np.int32)
    coeffs_h = np.where(np.repeat(ok, np.diff(batch.seg_offsets))[:, None, None], out["coeffs"], np.nan)
    errs, o, seg = _check_against_torch(gpu_ctx, batch, np.nan_to_num(coeffs_h), out["times"], 100, no, 9 + no, "mixed 8192",
                                        status=None)
    assert np.all(np.isfinite(errs[ok]))
    assert errs[ok].max() <= TOL_WELL
    # with the statuses and NaN in the coefficients of the failed paths: zero rows there, the same bits elsewhere
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        rng = np.random.default_rng(9 + no)
        q = _dev(_random_queries(rng, batch.seg_offsets, out["times"], 100))
        G = _dev(rng.standard_normal((batch.n_paths, 100, no, 4)))
        G[_dev(seg < 0)] = NAN
        o2 = _vjp(plan, _dev(coeffs_h), _dev(out["times"]), q, G, status=status)
    finally:
        plan.close()
    seg_ok = np.repeat(ok, np.diff(batch.seg_offsets))
    assert np.array_equal(o2["gc"][seg_ok], o["gc"][seg_ok]) and np.array_equal(o2["gt"][seg_ok], o["gt"][seg_ok])
    assert np.array_equal(o2["gq"][ok], o["gq"][ok])
    assert np.all(o2["gc"][~seg_ok] == 0.0) and np.all(o2["gt"][~seg_ok] == 0.0) and np.all(o2["gq"][~ok] == 0.0)


def test_gradcheck_of_autograd_evaluate_in_all_three_inputs(gpu_ctx):
    """Finite differences mean something where no query changes its segment and no heading crosses the seam under the
    perturbation: segment times of 1 .. 1.3 s, every query at least 1e-2 s inside its segment and every evaluated heading at
    least 1e-2 from +-pi (asserted); one query per path is negative (out of range: a zero row, no gradient)."""
    batch = pr.random_batch(4, 4, seed0=74000)
    rng = np.random.default_rng(3)
    t = 1.0 + 0.3 * rng.random(batch.n_segments)
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    Q = 9
    qh = np.zeros((4, Q))
    for p in range(4):
        edges = np.concatenate([[0.0], np.cumsum(t[so[p]:so[p + 1]])])
        i = rng.integers(0, 4, size=Q)
        qh[p] = edges[i] + rng.uniform(0.05, 0.95, size=Q) * (edges[i + 1] - edges[i])
    qh[:, 4] = -1.0
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask, fv0, times0, q0 = _dev(batch.fixed_mask), _dev(batch.fixed_values), _dev(t), _dev(qh)
    try:
        coeffs0, _, status = autograd.solve(plan, mask, fv0, times0)
        s0, seg0 = autograd.evaluate(plan, coeffs0, times0, q0, 5, status)
        torch.cuda.synchronize()
        assert bool(torch.all(status > 0)) and not seg0.requires_grad and seg0.dtype == torch.int32
        assert bool(torch.all(seg0[:, 4] == -1)) and int((seg0 >= 0).sum()) == 4 * (Q - 1)
        assert float(s0[:, :, 0, 3].abs().max()) < np.pi - 1e-2
        coeffs = coeffs0.detach().clone().requires_grad_(True)
        times = times0.clone().requires_grad_(True)
        q = q0.clone().requires_grad_(True)
        for no in (1, 5):
            assert torch.autograd.gradcheck(lambda c, tt, qq: autograd.evaluate(plan, c, tt, qq, no)[0], (coeffs, times, q),
                                            eps=1e-5, atol=1e-5, rtol=1e-3)
        fv = fv0.clone().requires_grad_(True)

        def chain(v, tt, qq):
            c, _, st = autograd.solve(plan, mask, v, tt)
            return autograd.evaluate(plan, c, tt, qq, 1, st)[0]
        assert torch.autograd.gradcheck(chain, (fv, times, q), eps=1e-5, atol=1e-5, rtol=1e-3)
        with pytest.raises(ValueError):
            autograd.evaluate(plan, coeffs, times, q, 3)
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()


def test_composite_fixtures_through_solve_and_evaluate(gpu_ctx):
    for case in eu.load_composite_cases():
        S, d, no = len(case["seg_times"]), case["derivative_to_optimize"], case["n_orders"]
        plan = api.Plan(gpu_ctx, np.array([0, S], dtype=np.int32))
        try:
            fv = _dev(np.array(case["fixed_values"], dtype=np.float64)).requires_grad_(True)
            times = _dev(case["seg_times"]).requires_grad_(True)
            q = _dev(np.array(case["query_times"])[None, :]).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, _dev(np.array(case["fixed_mask"]), np.uint8), fv, times, derivative=d)
            states, seg = autograd.evaluate(plan, coeffs, times, q, no, status)
            (states * _dev(np.array(case["grad_states"])[None])).sum().backward()
            torch.cuda.synchronize()
            gpu_ctx.use_torch_stream()
        finally:
            plan.close()
        assert int(status[0]) > 0 and np.array_equal(seg[0].cpu().numpy(), np.array(case["query_segment"]))
        rv, rt, rq = np.array(case["grad_fixed_values"]), np.array(case["grad_seg_times"]), np.array(case["grad_query_times"])
        scale = max(np.max(np.abs(rv)), np.max(np.abs(rt)), np.max(np.abs(rq)))
        e = max(np.max(np.abs(fv.grad.cpu().numpy() - rv)), np.max(np.abs(times.grad.cpu().numpy() - rt)),
                np.max(np.abs(q.grad.cpu().numpy()[0] - rq))) / scale
        print("EVALUATE GPU COMPOSITE %s: %.1e" % (case["name"], e))
        assert e <= (TOL_ILL if case["name"] == ILL_CASE else TOL_WELL), (case["name"], e)


def test_shuffled_queries_permute_the_outputs(gpu_ctx):
    batch = pr.random_batch(256, "ragged", seed0=75000)
    out = gpu_ctx.solve_batch(batch, None)
    rng = np.random.default_rng(21)
    Q = 200
    qh = np.sort(_random_queries(rng, batch.seg_offsets, out["times"], Q), axis=1)   # (NaN last)
    Gh = rng.standard_normal((256, Q, 5, 4))
    perm = np.stack([rng.permutation(Q) for _ in range(256)])
    rows = np.arange(256)[:, None]
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t = _dev(out["coeffs"]), _dev(out["times"])
        st, seg, tau = _eval(plan, c, t, _dev(qh), 5)
        o = _vjp(plan, c, t, _dev(qh), _dev(Gh))
        st2, seg2, tau2 = _eval(plan, c, t, _dev(qh[rows, perm]), 5)
        o2 = _vjp(plan, c, t, _dev(qh[rows, perm]), _dev(Gh[rows, perm]))
    finally:
        plan.close()
    assert np.array_equal(st2, st[rows, perm]) and np.array_equal(seg2, seg[rows, perm]) and np.array_equal(tau2, tau[rows, perm])
    assert np.array_equal(o2["gq"], o["gq"][rows, perm])
    scale = max(np.max(np.abs(o["gc"])), np.max(np.abs(o["gt"])))
    e = max(_rel(o2["gc"], o["gc"], scale), _rel(o2["gt"], o["gt"], scale))
    print("EVALUATE VJP GPU shuffled vs sorted queries: %.1e (bit-identical %s)" %
          (e, np.array_equal(o2["gc"], o["gc"]) and np.array_equal(o2["gt"], o["gt"])))
    assert e <= 1e-13   # (the order of every sum changed)


def test_repeats_streams_and_batch_position_give_the_same_bits(gpu_ctx):
    batch = pr.random_batch(300, "ragged", seed0=76000)
    out = gpu_ctx.solve_batch(batch, None)
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    rng = np.random.default_rng(22)
    Q = 130
    qh = _random_queries(rng, batch.seg_offsets, out["times"], Q)
    Gh = rng.standard_normal((300, Q, 5, 4))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t, q, G = _dev(out["coeffs"]), _dev(out["times"]), _dev(qh), _dev(Gh)
        a, b = _vjp(plan, c, t, q, G), _vjp(plan, c, t, q, G)
        sa, sb = _eval(plan, c, t, q, 5), _eval(plan, c, t, q, 5)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
        # through autograd on another stream
        cc, tt, qq = c.clone().requires_grad_(True), t.clone().requires_grad_(True), q.clone().requires_grad_(True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.default_stream())
        with torch.cuda.stream(s):
            st, _ = autograd.evaluate(plan, cc, tt, qq, 5)
            (st * G).sum().backward()
        torch.cuda.synchronize()
        assert np.array_equal(st.detach().cpu().numpy(), sa[0])
        assert np.array_equal(cc.grad.cpu().numpy(), a["gc"]) and np.array_equal(tt.grad.cpu().numpy(), a["gt"])
        assert np.array_equal(qq.grad.cpu().numpy(), a["gq"])
        gpu_ctx.use_torch_stream()
    finally:
        plan.close()
    # paths 17 and 250 as a batch of their own, in the other order
    pick = [250, 17]
    rows = np.concatenate([np.arange(so[p], so[p + 1]) for p in pick])
    so2 = np.concatenate([[0], np.cumsum([so[p + 1] - so[p] for p in pick])]).astype(np.int32)
    plan2 = api.Plan(gpu_ctx, so2)
    try:
        c2, t2 = _dev(out["coeffs"][rows]), _dev(out["times"][rows])
        o2 = _vjp(plan2, c2, t2, _dev(qh[pick]), _dev(Gh[pick]))
        s2 = _eval(plan2, c2, t2, _dev(qh[pick]), 5)
    finally:
        plan2.close()
    assert np.array_equal(o2["gc"], a["gc"][rows]) and np.array_equal(o2["gt"], a["gt"][rows])
    assert np.array_equal(o2["gq"], a["gq"][pick])
    for x, y in zip(s2, sa):
        assert np.array_equal(x, y[pick])


def test_degenerate_paths_and_arguments(gpu_ctx):
    batch = pr.random_batch(6, 5, seed0=77000)
    out = gpu_ctx.solve_batch(batch, None)
    rng = np.random.default_rng(23)
    Q = 70
    qh = _random_queries(rng, batch.seg_offsets, out["times"], Q)
    Gh = rng.standard_normal((6, Q, 5, 4))
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t, q, G = _dev(out["coeffs"]), _dev(out["times"]), _dev(qh), _dev(Gh)
        ref = _vjp(plan, c, t, q, G)
        st, seg, tau = _eval(plan, c, t, q, 5)
        assert np.any(seg < 0) and np.all(ref["gq"][seg < 0] == 0.0)
        # NaN upstream rows of out-of-range queries change nothing
        Gn = Gh.copy()
        Gn[seg < 0] = np.nan
        o = _vjp(plan, c, t, q, _dev(Gn))
        for k in ref:
            assert np.array_equal(o[k], ref[k]), k
        # status <= 0 with NaN coefficients: zero rows in all three outputs, the other paths' bits untouched
        ch = out["coeffs"].copy()
        ch[5:10] = np.nan
        status = np.ones(6, dtype=np.int32)
        status[1] = -2
        o = _vjp(plan, _dev(ch), t, q, G, status=_dev(status))
        assert np.all(o["gc"][5:10] == 0.0) and np.all(o["gt"][5:10] == 0.0) and np.all(o["gq"][1] == 0.0)
        keep = np.r_[0:5, 10:30]
        assert np.array_equal(o["gc"][keep], ref["gc"][keep]) and np.array_equal(o["gt"][keep], ref["gt"][keep])
        assert np.array_equal(o["gq"][[0, 2, 3, 4, 5]], ref["gq"][[0, 2, 3, 4, 5]])
        # a path whose total time is not a number: every query out of range, zero rows
        th = out["times"].copy()
        th[12] = np.nan
        s3, seg3, _ = _eval(plan, c, _dev(th), q, 5)
        o = _vjp(plan, c, _dev(th), q, G)
        assert np.all(seg3[2] == -1) and np.all(s3[2] == 0.0)
        assert np.all(o["gc"][10:15] == 0.0) and np.all(o["gt"][10:15] == 0.0) and np.all(o["gq"][2] == 0.0)
        keep = np.r_[0:10, 15:30]
        assert np.array_equal(o["gc"][keep], ref["gc"][keep]) and np.array_equal(seg3[[0, 1, 3, 4, 5]], seg[[0, 1, 3, 4, 5]])
        # each output on its own gives the bits of all three together
        for k in ref:
            assert np.array_equal(_vjp(plan, c, t, q, G, want=(k,))[k], ref[k]), k
        # one order is order 0 of five
        s1, seg1, tau1 = _eval(plan, c, t, q, 1)
        assert np.array_equal(s1[:, :, 0], st[:, :, 0]) and np.array_equal(seg1, seg) and np.array_equal(tau1, tau)
        # no queries: succeeds; the backward still writes zeros
        q0 = torch.zeros((6, 0), dtype=torch.float64, device="cuda")
        plan.evaluate(c, t, q0, torch.zeros((6, 0, 5, 4), dtype=torch.float64, device="cuda"))
        o = _vjp(plan, c, t, q0, torch.zeros((6, 0, 5, 4), dtype=torch.float64, device="cuda"))
        assert np.all(o["gc"] == 0.0) and np.all(o["gt"] == 0.0) and o["gq"].shape == (6, 0)
        # invalid calls: the error code and a message
        L, h = plan._L, plan._h
        p = lambda x: None if x is None else x.data_ptr()   # noqa: E731
        states = torch.zeros((6, Q, 5, 4), dtype=torch.float64, device="cuda")
        gc = torch.zeros((30, 4, 10), dtype=torch.float64, device="cuda")
        bad = [L.mrs_tg_plan_evaluate(h, p(c), p(t), p(q), Q, 3, p(states), None, None),        # n_orders 3
               L.mrs_tg_plan_evaluate(h, p(c), p(t), p(q), -1, 5, p(states), None, None),       # negative count
               L.mrs_tg_plan_evaluate(h, p(c), p(t), p(q), Q, 5, None, None, None),             # no states
               L.mrs_tg_plan_evaluate(h, p(c), p(t), None, Q, 5, p(states), None, None),        # no queries
               L.mrs_tg_plan_evaluate(h, None, p(t), p(q), Q, 5, p(states), None, None),        # no coefficients
               L.mrs_tg_plan_evaluate(None, p(c), p(t), p(q), Q, 5, p(states), None, None),     # no plan
               L.mrs_tg_plan_evaluate_vjp(h, p(c), p(t), p(q), Q, 5, p(G), None, None, None, None),      # no output
               L.mrs_tg_plan_evaluate_vjp(h, p(c), p(t), p(q), Q, 5, None, None, p(gc), None, None),     # no upstream
               L.mrs_tg_plan_evaluate_vjp(h, p(c), p(t), p(q), Q, 2, p(G), None, p(gc), None, None),     # n_orders 2
               L.mrs_tg_plan_evaluate_vjp(h, p(c), p(t), p(q), -5, 5, p(G), None, p(gc), None, None),    # negative count
               L.mrs_tg_plan_evaluate_vjp(h, p(c), None, p(q), Q, 5, p(G), None, p(gc), None, None)]     # no times
        assert all(rc == ERR_INVALID_ARG for rc in bad), bad
        with pytest.raises(api.MrsTgError) as err:
            plan.evaluate(c, t, q, states[:, :, :3].contiguous())
        assert "n_orders" in str(err.value)
        with pytest.raises(api.MrsTgError) as err:
            plan.evaluate_vjp(c, t, q, G)
        assert "NULL" in str(err.value)
    finally:
        plan.close()


def test_a_200_segment_path_and_100000_queries_agree_with_the_harness(gpu_ctx, tmp_path):
    exe = eu.build_harness(tmp_path)
    rng = np.random.default_rng(31)
    # one path of 200 segments next to a short one
    S = 200
    T = rng.uniform(0.2, 1.0, size=S + 3)
    T[57] = 0.0
    cf = rng.standard_normal((S + 3, 4, 10)) * 0.5 ** np.arange(10)
    so = np.array([0, S, S + 3], dtype=np.int32)
    Q = 333
    qh = _random_queries(rng, so, T, Q)
    qh[0, 2:S + 2] = np.cumsum(T[:S])   # (every vertex as numpy sums it: on or next to the double-precision running sum)
    Gh = rng.standard_normal((2, Q, 5, 4))
    plan = api.Plan(gpu_ctx, so)
    try:
        c, t, q = _dev(cf), _dev(T), _dev(qh)
        st, seg, tau = _eval(plan, c, t, q, 5)
        Gh[seg < 0] = np.nan
        o = _vjp(plan, c, t, q, _dev(Gh))
    finally:
        plan.close()
    cpu = eu.run_harness(exe, [dict(seg_times=T[a:b], coeffs=cf[a:b], query_times=qh[p], n_orders=5, grad_states=np.nan_to_num(Gh[p]))
                               for p, (a, b) in enumerate(zip(so[:-1], so[1:]))])
    for p, (a, b) in enumerate(zip(so[:-1], so[1:])):
        h = cpu[p]
        assert np.array_equal(seg[p], h["query_segment"]) and np.array_equal(tau[p], h["query_local_time"])
        assert _rel(st[p], h["states"], np.max(np.abs(h["states"]))) <= TOL_GPU_CPU
        gs = max(np.max(np.abs(h["grad_coeffs"])), np.max(np.abs(h["grad_seg_times"])), np.max(np.abs(h["grad_query_times"])))
        e = max(_rel(o["gc"][a:b], h["grad_coeffs"], gs), _rel(o["gt"][a:b], h["grad_seg_times"], gs),
                _rel(o["gq"][p], h["grad_query_times"], gs))
        print("EVALUATE GPU %d segments vs CPU harness: %.1e, bit-identical %s" %
              (b - a, e, np.array_equal(o["gc"][a:b], h["grad_coeffs"]) and np.array_equal(st[p], h["states"])))
        assert e <= TOL_GPU_CPU
    assert 57 not in seg[0] and seg[0].max() == S - 1
    # 100 000 queries on each of 4 paths (the forward cuts them into slices; the backward streams them)
    batch = pr.random_batch(4, 7, seed0=78000)
    out = gpu_ctx.solve_batch(batch, None)
    Q = 100000
    qh = _random_queries(rng, batch.seg_offsets, out["times"], Q)
    Gh = rng.integers(-64, 65, size=(4, Q, 1, 4)) / 64.0
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        c, t, q = _dev(out["coeffs"]), _dev(out["times"]), _dev(qh)
        st, seg, tau = _eval(plan, c, t, q, 1)
        o = _vjp(plan, c, t, q, _dev(Gh))
    finally:
        plan.close()
    assert np.all(seg >= -1) and np.all(np.isfinite(st)) and np.all(np.isfinite(o["gq"]))
    so = np.asarray(batch.seg_offsets)
    for p in (0, 3):
        a, b = so[p], so[p + 1]
        h = eu.run_harness(exe, [dict(seg_times=out["times"][a:b], coeffs=out["coeffs"][a:b], query_times=qh[p], n_orders=1,
                                      grad_states=Gh[p])])[0]
        assert np.array_equal(seg[p], h["query_segment"]) and np.array_equal(tau[p], h["query_local_time"])
        assert _rel(st[p], h["states"], np.max(np.abs(h["states"]))) <= TOL_GPU_CPU
        gs = max(np.max(np.abs(h["grad_coeffs"])), np.max(np.abs(h["grad_seg_times"])), np.max(np.abs(h["grad_query_times"])))
        e = max(_rel(o["gc"][a:b], h["grad_coeffs"], gs), _rel(o["gt"][a:b], h["grad_seg_times"], gs),
                _rel(o["gq"][p], h["grad_query_times"], gs))
        print("EVALUATE GPU 100000 queries, path %d vs CPU harness: %.1e, bit-identical %s" %
              (p, e, np.array_equal(o["gc"][a:b], h["grad_coeffs"]) and np.array_equal(st[p], h["states"])))
        assert e <= TOL_GPU_CPU

"""mrs_tg_plan_request_vertices, mrs_tg_plan_request_limits and their backward passes on the GPU (mrs_tg_request.hip, DESIGN.md
section 11h), with the autograd functions on top of them.  Everything is compared bit for bit: the vertices against
problem.build_vertices per path (the unwrap is fmod, additions and comparisons), the limits and the branch word against the CPU
harness's output (tests/host/request_harness.cpp; the hypot edges are Pythagorean, exact on both sides), the backward passes
against torch's autograd on index and torch.where restatements, and the chain request -> limits + vertices -> times -> solve ->
samples -> loss against the same chain with the new backward passes called by hand.  P <= 32 paths throughout."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api
from mrs_uav_trajectory_generation_amd import autograd as ag
from mrs_uav_trajectory_generation_amd import problem as pr
from tests import request_util as ru

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one path per V: the chunk edges, two chunks, MRS_TG_MAX_SEGMENTS + 1 vertices
RAGGED_V = (2, 3, 4, 11, 63, 64, 65, 66, 128, 129, 130, 257)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ru.build_harness(tmp_path_factory.mktemp("request_gpu"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _initial_state(q):
    s = q["state"]
    return dict(heading=float(s[0, 3]), velocity=s[1], acceleration=s[2], jerk=s[3])


def _reference(problems, d, with_stop=True, with_state=True):
    """problem.build_vertices per path, concatenated"""
    parts = [pr.build_vertices(q["raw"], d, stop_at=q["stop"] if with_stop else None,
                               initial_state=_initial_state(q) if with_state and q["has"] else None) for q in problems]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _run_vertices(plan, ctx, problems, d, in_place=False, with_stop=True, with_state=True):
    raw = _dev(np.concatenate([q["raw"] for q in problems]))
    n_v = raw.shape[0]
    stop = _dev(np.concatenate([q["stop"] for q in problems])) if with_stop else None
    has = _dev(np.array([q["has"] for q in problems], dtype=np.uint8)) if with_state else None
    state = _dev(np.stack([q["state"] for q in problems])) if with_state else None
    out = raw if in_place else torch.full((n_v, 4), float("nan"), dtype=torch.float64, device=DEV)
    mask = torch.full((n_v, 5), 0xFF, dtype=torch.uint8, device=DEV)
    vals = torch.full((n_v, 5, 4), float("nan"), dtype=torch.float64, device=DEV)
    plan.request_vertices(raw, out, mask, vals, stop_at=stop, has_state=has, state=state, derivative_to_optimize=d)
    ctx.synchronize()
    return out.cpu().numpy(), mask.cpu().numpy(), vals.cpu().numpy()


def _check_vertices(ctx, problems, d):
    so = np.concatenate([[0], np.cumsum([q["V"] - 1 for q in problems])]).astype(np.int32)
    plan = api.Plan(ctx, so)
    try:
        for kw in (dict(), dict(in_place=True), dict(with_stop=False), dict(with_state=False)):
            got = _run_vertices(plan, ctx, problems, d, **kw)
            want = _reference(problems, d, with_stop=kw.get("with_stop", True), with_state=kw.get("with_state", True))
            first = np.concatenate([[0], np.cumsum([q["V"] for q in problems])])
            for name, g, w in zip(("waypoints", "mask", "values"), got, want):
                if _bits(g) != _bits(w):
                    bad = [q["V"] for p, q in enumerate(problems) if _bits(g[first[p]:first[p + 1]]) != _bits(w[first[p]:first[p + 1]])]
                    pytest.fail("%s differ for d = %d, %r, paths of %r vertices" % (name, d, kw, bad))
    finally:
        plan.close()


def test_capability_bit_abi_version_and_kernel_ids(gpu_ctx):
    assert api.capabilities() & api.CAP_REQUEST and api.CAP_REQUEST == 32768
    lib = api.load_library()
    assert lib.mrs_tg_abi_version() == 5
    assert (api.REQ_OVERRIDE, api.REQ_RELAX_HEADING) == (1, 2)
    assert (api.LIM_OVERRIDDEN, api.LIM_OVERRIDE_REFUSED, api.LIM_RELAXED, api.LIM_V_DESCENDING, api.LIM_A_DESCENDING,
            api.LIM_J_DESCENDING, api.LIM_FALLBACK) == (1, 2, 4, 8, 16, 32, 64)
    for name in ("mrs_tg_plan_request_vertices", "mrs_tg_plan_request_vertices_vjp", "mrs_tg_plan_request_limits",
                 "mrs_tg_plan_request_limits_vjp"):
        assert hasattr(lib, name) and name in api.EXPORTED_SYMBOLS
    rng = np.random.default_rng(1)
    problems = [ru.vertex_problem(rng, 5, 4, p % 2) for p in range(4)]
    P, n_v = 4, 20
    plan = api.Plan(gpu_ctx, np.arange(P + 1, dtype=np.int32) * 4)
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        _run_vertices(plan, gpu_ctx, problems, 4)
        g = torch.ones((n_v, 4), dtype=torch.float64, device=DEV)
        plan.request_vertices_vjp(g, None, torch.empty_like(g), None)
        c = _dev(np.tile(ru.constraints("<<<"), (P, 1)))
        lim = torch.empty((P, 9), dtype=torch.float64, device=DEV)
        branch = torch.empty(P, dtype=torch.int32, device=DEV)
        plan.request_limits(c, lim, branch)
        plan.request_limits_vjp(branch, lim, torch.empty_like(c))
        mine = ("request_vertices_kernel", "request_vertices_vjp_kernel", "request_limits_kernel", "request_limits_vjp_kernel")
        assert tuple(k for k in api.kernel_trace() if k in mine) == mine, api.kernel_trace()
        for kernel in (api.KERNEL_REQUEST_VERTICES, api.KERNEL_REQUEST_VERTICES_VJP, api.KERNEL_REQUEST_LIMITS,
                       api.KERNEL_REQUEST_LIMITS_VJP):
            assert gpu_ctx.last_kernel_ms(kernel) > 0, kernel
        # the argument checks
        wp = torch.zeros((n_v, 4), dtype=torch.float64, device=DEV)
        has = torch.ones(P, dtype=torch.uint8, device=DEV)
        for call in (lambda: plan.request_vertices(wp, wp, derivative_to_optimize=1),
                     lambda: plan.request_vertices(wp, wp, derivative_to_optimize=5),
                     lambda: plan.request_vertices(wp, wp, has_state=has),
                     lambda: plan.request_vertices(wp),
                     lambda: plan.request_vertices_vjp(None, None, g, None),
                     lambda: plan.request_vertices_vjp(g, None, None, None),
                     lambda: plan.request_limits(c, lim, flags=branch),
                     lambda: plan.request_limits(c, lim, has_state=has),
                     lambda: plan.request_limits(c),
                     lambda: plan.request_limits_vjp(branch, None, c),
                     lambda: plan.request_limits_vjp(branch, lim)):
            with pytest.raises(api.MrsTgError):
                call()
    finally:
        gpu_ctx.set_profiling(False)
        plan.close()


@pytest.mark.parametrize("d", (2, 3, 4))
def test_vertices_of_a_ragged_batch_have_the_bytes_of_build_vertices(gpu_ctx, d):
    rng = np.random.default_rng(30 + d)
    problems = [ru.vertex_problem(rng, V, d, p % 2, pi_steps=(p % 3 == 2)) for p, V in enumerate(RAGGED_V)]
    _check_vertices(gpu_ctx, problems, d)


@pytest.mark.parametrize("d", (2, 3, 4))
def test_vertices_of_a_uniform_batch_have_the_bytes_of_build_vertices(gpu_ctx, d):
    rng = np.random.default_rng(40 + d)
    problems = [ru.vertex_problem(rng, 11, d, p % 2) for p in range(8)]
    _check_vertices(gpu_ctx, problems, d)


def test_vertices_backward_against_torch_autograd(gpu_ctx):
    rng = np.random.default_rng(50)
    counts = np.array([2, 3, 4, 11, 65, 7])
    P, n_v = counts.size, int(counts.sum())
    so = np.concatenate([[0], np.cumsum(counts - 1)]).astype(np.int32)
    first = _dev(np.concatenate([[0], np.cumsum(counts)])[:-1])
    has_np = np.array([1, 0, 1, 1, 0, 1], dtype=bool)
    g_wp = _dev(rng.integers(-128, 129, (n_v, 4)) / 64.0)
    g_vals = _dev(rng.integers(-128, 129, (n_v, 5, 4)) / 64.0)
    plan = api.Plan(gpu_ctx, so)
    try:
        for has in (has_np, None):
            for up_wp, up_vals in ((g_wp, g_vals), (g_wp, None), (None, g_vals)):
                wp = _dev(rng.uniform(-3.0, 3.0, (n_v, 4))).requires_grad_()
                st = _dev(rng.uniform(-3.0, 3.0, (P, 4, 4))).requires_grad_()
                vals = torch.zeros((n_v, 5, 4), dtype=torch.float64, device=DEV)
                vals = torch.cat([wp[:, None, :], vals[:, 1:]], dim=1)
                if has is not None:
                    at = first[_dev(has)]
                    rows = torch.zeros((n_v, 5, 4), dtype=torch.float64, device=DEV)
                    rows = rows.index_put((at,), torch.cat([torch.zeros_like(st[:, :1]), st[:, 1:], torch.zeros_like(st[:, :1])],
                                                            dim=1)[_dev(has)])
                    vals = vals + rows
                loss = (wp * up_wp).sum() if up_wp is not None else 0.0
                loss = loss + ((vals * up_vals).sum() if up_vals is not None else 0.0)
                loss.backward()
                want_wp = wp.grad
                want_st = st.grad if st.grad is not None else torch.zeros_like(st)
                has_d = None if has is None else _dev(has.astype(np.uint8))
                for give_wp, give_st in ((True, True), (True, False), (False, True)):
                    got_wp = torch.full((n_v, 4), float("nan"), dtype=torch.float64, device=DEV) if give_wp else None
                    got_st = torch.full((P, 4, 4), float("nan"), dtype=torch.float64, device=DEV) if give_st else None
                    plan.request_vertices_vjp(up_wp, up_vals, got_wp, got_st, has_state=has_d)
                    gpu_ctx.synchronize()
                    if give_wp:
                        assert torch.equal(got_wp, want_wp)
                    if give_st:
                        assert torch.equal(got_st, want_st)
                        assert not bool(got_st[:, 0].any())
                if has is not None and up_vals is not None:
                    assert bool(want_st[_dev(has)][:, 1:].abs().sum() > 0) and not bool(want_st[_dev(~has)].any())
    finally:
        plan.close()


def _limit_batches():
    """the CPU test's branch table and edges, by fallback (one scalar per call), in batches of 32 and a remainder"""
    rows = ru.limits_table() + ru.edge_rows()
    for fallback in (0, 1):
        mine = [r for r in rows if r["fallback"] == fallback]
        for b0 in range(0, len(mine), 32):
            yield fallback, mine[b0:b0 + 32]


def _run_limits(ctx, rows, fallback):
    P = len(rows)
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    try:
        c, o = _dev(np.stack([r["c"] for r in rows])), _dev(np.stack([r["o"] for r in rows]))
        flags = _dev(np.array([r["flags"] for r in rows], dtype=np.int32))
        has = _dev(np.array([r["has"] for r in rows], dtype=np.uint8))
        state = _dev(np.stack([r["state"] for r in rows]))
        lim = torch.full((P, 9), float("nan"), dtype=torch.float64, device=DEV)
        branch = torch.full((P,), -1, dtype=torch.int32, device=DEV)
        plan.request_limits(c, lim, branch, override=o, flags=flags, has_state=has, state=state, fallback=bool(fallback),
                            speed_factor=ru.SPEED_FACTOR, accel_factor=ru.ACCEL_FACTOR)
        ctx.synchronize()
        return c, o, lim, branch, plan
    except Exception:
        plan.close()
        raise


def test_limits_branch_table_has_the_bytes_of_the_harness(gpu_ctx, harness):
    sizes, seen = [], set()
    for fallback, rows in _limit_batches():
        sizes.append(len(rows))
        want_branch, want_lim, _ = ru.run_limits(harness, rows)
        c, o, lim, branch, plan = _run_limits(gpu_ctx, rows, fallback)
        plan.close()
        assert _bits(lim.cpu().numpy()) == _bits(want_lim), (fallback, lim.cpu().numpy() - want_lim)
        assert branch.cpu().numpy().tolist() == want_branch.tolist() == [r["expect"] for r in rows]
        seen |= set(want_branch.tolist())
    assert sizes == [32, 32, 32, 12, 32, 32, 32]
    assert any(w & ru.OVERRIDE_REFUSED for w in seen) and any(w & ru.OVERRIDDEN for w in seen) and any(w & ru.RELAXED for w in seen)


def _limits_torch(c, o, branch, fallback):
    """the forward as torch.where over the branch word"""
    over = (branch & ru.OVERRIDDEN) != 0
    relaxed = (branch & ru.RELAXED) != 0
    flt_max = torch.full_like(c[:, 0], ru.FLT_MAX)

    def pair(asc, bit):
        return torch.where((branch & bit) != 0, c[:, asc + 1], c[:, asc])
    cols = [torch.where(over, o[:, 0], c[:, 0]), torch.where(over, o[:, 1], pair(3, ru.V_DESCENDING)), torch.where(relaxed, flt_max, c[:, 9]),
            torch.where(over, o[:, 2], c[:, 1]), torch.where(over, o[:, 3], pair(5, ru.A_DESCENDING)), torch.where(relaxed, flt_max, c[:, 10]),
            torch.where(over, o[:, 4], c[:, 2]), torch.where(over, o[:, 5], pair(7, ru.J_DESCENDING)), torch.where(relaxed, flt_max, c[:, 11])]
    if fallback:
        cols[0], cols[1] = cols[0] * ru.SPEED_FACTOR, cols[1] * ru.SPEED_FACTOR
        cols[3], cols[4] = cols[3] * ru.ACCEL_FACTOR, cols[4] * ru.ACCEL_FACTOR
    return torch.stack(cols, dim=1)


def test_limits_backward_against_torch_autograd(gpu_ctx):
    rng = np.random.default_rng(60)
    for fallback, rows in _limit_batches():
        P = len(rows)
        c, o, lim, branch, plan = _run_limits(gpu_ctx, rows, fallback)
        try:
            c, o = c.clone().requires_grad_(), o.clone().requires_grad_()
            again = _limits_torch(c, o, branch, fallback)
            assert torch.equal(again.detach(), lim)
            g = _dev(rng.integers(-128, 129, (P, 9)) / 64.0)
            (again * g).sum().backward()
            for give_c, give_o in ((True, True), (True, False), (False, True)):
                gc = torch.full((P, 12), float("nan"), dtype=torch.float64, device=DEV) if give_c else None
                go = torch.full((P, 6), float("nan"), dtype=torch.float64, device=DEV) if give_o else None
                plan.request_limits_vjp(branch, g, gc, go, fallback=bool(fallback), speed_factor=ru.SPEED_FACTOR,
                                        accel_factor=ru.ACCEL_FACTOR)
                gpu_ctx.synchronize()
                assert gc is None or torch.equal(gc, c.grad)
                assert go is None or torch.equal(go, o.grad)
        finally:
            plan.close()


def test_chain_from_the_raw_request_to_a_loss_on_the_samples(gpu_ctx):
    """request_limits + request_vertices -> estimate_times -> solve -> sample -> quadratic loss through autograd, against the
    same chain cut at the two new steps with their backward passes called by hand: bit for bit."""
    rng = np.random.default_rng(70)
    cap = 512
    counts = np.array([3, 6, 2, 4])
    P, n_v = counts.size, int(counts.sum())
    so = np.concatenate([[0], np.cumsum(counts - 1)]).astype(np.int32)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    raw_np = np.concatenate([np.cumsum(rng.uniform(1.5, 3.0, (n, 4)), axis=0) for n in counts])
    raw_np[:, 3] = rng.uniform(-0.3, 0.3, n_v) + 2.0 * np.pi * rng.integers(-1, 2, n_v)      # raw headings: whole turns apart
    st_np = rng.uniform(-0.5, 0.5, (P, 4, 4))
    st_np[:, 0, 3] = raw_np[first, 3] + 2.0 * np.pi                                          # the chain shifts every path
    has = _dev(np.array([1, 1, 0, 1], dtype=np.uint8))
    c_np = np.tile(np.array([2.0, 2.0, 20.0, 2.0, 3.0, 2.5, 2.0, 20.0, 25.0, 1.0, 2.0, 20.0]), (P, 1))
    target = _dev(rng.uniform(0.0, 10.0, (P, cap, 4)))
    plan = api.Plan(gpu_ctx, so)

    def tail(wp, mask, fv, lim):
        times = ag.estimate_times(plan, wp, lim)
        coeffs, _, status = ag.solve(plan, mask, fv, times)
        samples, n = ag.sample(plan, coeffs, times, 0.2, cap, status)
        valid = (torch.arange(cap, device=DEV)[None, :] < n[:, None])[:, :, None]
        return (((samples - target) ** 2) * valid).sum(), status, n

    try:
        # (1) autograd all the way
        raw, st, c = _dev(raw_np).requires_grad_(), _dev(st_np).requires_grad_(), _dev(c_np).requires_grad_()
        lim, branch = ag.request_limits(plan, c, state=st, has_state=has, return_branch=True)
        wp, mask, fv = ag.request_vertices(plan, raw, state=st, has_state=has)
        assert bool(((wp - raw).detach()[:, 3].abs() > 6.0).any())
        loss, status, n = tail(wp, mask, fv, lim)
        assert bool((status > 0).all()) and bool((n > 2).all())
        loss.backward()
        assert raw.grad is not None and st.grad is not None and c.grad is not None
        assert bool(st.grad[:, 1].abs().sum() > 0) and bool(raw.grad.abs().sum() > 0) and bool(c.grad.abs().sum() > 0)
        assert not bool(st.grad[:, 0].any()) and not bool(st.grad[2].any())

        # (2) the same chain, cut at the new steps
        lim2 = torch.empty((P, 9), dtype=torch.float64, device=DEV)
        branch2 = torch.empty(P, dtype=torch.int32, device=DEV)
        plan.request_limits(_dev(c_np), lim2, branch2, has_state=has, state=_dev(st_np))
        wp2, mask2, fv2 = torch.empty((n_v, 4), dtype=torch.float64, device=DEV), torch.empty((n_v, 5), dtype=torch.uint8, device=DEV), \
            torch.empty((n_v, 5, 4), dtype=torch.float64, device=DEV)
        plan.request_vertices(_dev(raw_np), wp2, mask2, fv2, has_state=has, state=_dev(st_np))
        assert torch.equal(lim2, lim.detach()) and torch.equal(branch2, branch) and torch.equal(wp2, wp.detach())
        assert torch.equal(mask2, mask) and torch.equal(fv2, fv.detach())
        wp_leaf, fv_leaf, lim_leaf = wp2.clone().requires_grad_(), fv2.clone().requires_grad_(), lim2.clone().requires_grad_()
        loss2, _, _ = tail(wp_leaf, mask2, fv_leaf, lim_leaf)
        assert torch.equal(loss2.detach(), loss.detach())
        g_wp, g_fv, g_lim = torch.autograd.grad(loss2, (wp_leaf, fv_leaf, lim_leaf))
        g_raw = torch.full((n_v, 4), float("nan"), dtype=torch.float64, device=DEV)
        g_st = torch.full((P, 4, 4), float("nan"), dtype=torch.float64, device=DEV)
        plan.request_vertices_vjp(g_wp.contiguous(), g_fv.contiguous(), g_raw, g_st, has_state=has)
        g_c = torch.full((P, 12), float("nan"), dtype=torch.float64, device=DEV)
        plan.request_limits_vjp(branch2, g_lim.contiguous(), g_c)
        gpu_ctx.synchronize()
        assert torch.equal(raw.grad, g_raw) and torch.equal(st.grad, g_st) and torch.equal(c.grad, g_c)
    finally:
        plan.close()

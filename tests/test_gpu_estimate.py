"""mrs_tg_plan_estimate_times / mrs_tg_plan_estimate_times_vjp on the GPU (estimate_times_kernel, estimate_times_vjp_kernel,
DESIGN.md section 4e) and autograd.estimate_times on top of them: the forward against the solve's own estimate bit for bit, the
backward pass against the 60-digit fixtures, against the CPU harness bit for bit and against central differences of the GPU
forward, and the wiring of the chain that starts at the waypoints.  NaN inputs are ordinary data here: nothing provokes a
fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd, problem as pr
from tests import deviation_util as du
from tests import estimate_util as eu
from tests import util

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
GENERAL = api.FLAG_GENERAL_PATTERNS


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return eu.build_harness(tmp_path_factory.mktemp("estimate_gpu"))


@pytest.fixture(scope="module")
def shapes():
    return eu.shapes()


def _guarded(rows, tail, dtype, fill):
    """a tensor with one guard row in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _forward(ctx, so, wp, lim):
    plan = api.Plan(ctx, so)
    try:
        full, view = _guarded(int(so[-1]), (), torch.float64, SENTINEL)
        plan.estimate_times(_dev(wp), _dev(lim), view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    host = full.cpu().numpy()
    assert host[0] == SENTINEL and host[-1] == SENTINEL
    return host[1:-1].copy()


def _backward(ctx, so, wp, lim, upstream, want=("grad_waypoints", "grad_limits", "term")):
    """one backward call -> host arrays by name; every output is prefilled with a sentinel and has guard rows on both sides"""
    P, nS = len(so) - 1, int(so[-1])
    spec = dict(grad_waypoints=(nS + P, (4,), torch.float64, SENTINEL), grad_limits=(P, (9,), torch.float64, SENTINEL),
                term=(nS, (), torch.int32, ISENTINEL))
    full, view = {}, {}
    for name in want:
        full[name], view[name] = _guarded(*spec[name])
    plan = api.Plan(ctx, so)
    try:
        plan.estimate_times_vjp(_dev(wp), _dev(lim), None if upstream is None else _dev(upstream), **view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    out = {}
    for name in want:
        host = full[name].cpu().numpy()
        fill = spec[name][3]
        assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
        assert not np.any(host[1:-1] == fill), "%s: an element of the plan was not written" % name
        out[name] = host[1:-1].copy()
    return out


def _compare_with_harness(out, probs, cpu, so):
    for q, (p, h) in enumerate(zip(probs, cpu)):
        a, b = int(so[q]), int(so[q + 1])
        assert np.array_equal(out["term"][a:b], h["term"]), q
        assert eu.same_bits(out["grad_waypoints"][a + q:b + q + 1], h["grad_waypoints"]), q
        assert eu.same_bits(out["grad_limits"][q], h["grad_limits"]), q


def test_the_library_reports_the_capability_and_times_both_kernels(gpu_ctx, shapes):
    assert api.CAP_ESTIMATE_GRADIENT == 256 and api.capabilities() & api.CAP_ESTIMATE_GRADIENT
    assert (api.ESTIMATE_TERM_HORIZONTAL, api.ESTIMATE_TERM_VERTICAL, api.ESTIMATE_TERM_FLOOR, api.ESTIMATE_TERM_HEADING) == \
        (eu.HORIZONTAL, eu.VERTICAL, eu.FLOOR, eu.HEADING) == (0, 1, 2, 3)
    assert (api.KERNEL_ESTIMATE, api.KERNEL_ESTIMATE_VJP) == (10, 11)
    so, wp, lim, g = eu.pack(eu.batch_problems(shapes["uniform_70x3"], 5))
    try:
        gpu_ctx.set_profiling(True)
        _forward(gpu_ctx, so, wp, lim)
        _backward(gpu_ctx, so, wp, lim, g)
        assert gpu_ctx.last_kernel_ms(api.KERNEL_ESTIMATE) > 0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_ESTIMATE_VJP) > 0
    finally:
        gpu_ctx.set_profiling(False)


@pytest.mark.parametrize("shape", ["uniform_3x1", "uniform_70x3", "mixed_70", "one_path"])
def test_forward_is_the_solves_own_estimate_in_the_same_bits(gpu_ctx, shapes, shape):
    batch = shapes[shape]
    times = _forward(gpu_ctx, batch.seg_offsets, batch.waypoints, batch.limits)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        t = torch.zeros(plan.n_segments, dtype=torch.float64, device="cuda")
        coeffs = torch.zeros((plan.n_segments, 4, 10), dtype=torch.float64, device="cuda")
        status = torch.zeros(plan.n_paths, dtype=torch.int32, device="cuda")
        opt = api.default_options(derivative_to_optimize=4, time_alloc_method=api.TIME_ALLOC_NONE, estimate_times=1,
                                  sampling_dt=0.0, flags=GENERAL)
        plan.solve(opt, _dev(batch.fixed_mask), _dev(batch.fixed_values), t, coeffs, status, waypoints=_dev(batch.waypoints),
                   limits=_dev(batch.limits))
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert eu.same_bits(times, t.cpu().numpy())
    ref = util.oracle_times(batch)
    assert np.all(np.abs(times - ref) <= eu.VALUE_RTOL * ref)


def test_fixture_through_the_gpu(gpu_ctx):
    cases = eu.load_cases()
    probs = [eu.case_problem(c) for c in cases]
    so, wp, lim, g = eu.pack(probs)
    times = _forward(gpu_ctx, so, wp, lim)
    out = _backward(gpu_ctx, so, wp, lim, g)
    report = {}
    for q, c in enumerate(cases):
        a, b = int(so[q]), int(so[q + 1])
        assert out["term"][a:b].tolist() == c["term"], c["name"]
        exact = np.array(c["value"])
        assert np.all(np.abs(times[a:b] - exact) <= eu.VALUE_RTOL * exact), c["name"]
        assert np.all(times[a:b][np.array(c["term"]) == eu.FLOOR] == 0.01), c["name"]
        ew, el, ratio = eu.gradient_excess(c, out["grad_waypoints"][a + q:b + q + 1], out["grad_limits"][q])
        report[c["name"]] = "%.2f" % ratio
        assert ew <= 0.0 and el <= 0.0, (c["name"], ew, el)
    print("ESTIMATE GPU GRADIENT FIXTURES, largest |error| / bound: %s" % report)


def test_gpu_gradients_and_terms_are_the_harness_in_bits(gpu_ctx, harness, shapes):
    groups = dict(fixture=[eu.case_problem(c) for c in eu.load_cases()])
    for n, (name, batch) in enumerate(shapes.items()):
        groups[name] = eu.batch_problems(batch, 10 + n)
    for name, probs in groups.items():
        so, wp, lim, g = eu.pack(probs)
        try:
            _compare_with_harness(_backward(gpu_ctx, so, wp, lim, g), probs, eu.run_harness(harness, probs), so)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
    mixed = shapes["mixed_70"]
    S = np.diff(mixed.seg_offsets)
    assert mixed.n_segments + mixed.n_paths > 256 and S.min() < 3 and S.max() > 25 and len(set(S.tolist())) > 10
    so, wp, lim, g = eu.pack(groups["mixed_70"])
    seen = set(_backward(gpu_ctx, so, wp, lim, g, want=("term",))["term"].tolist())
    assert {eu.HORIZONTAL, eu.VERTICAL, eu.HEADING} <= seen


def test_a_path_gives_the_same_bits_wherever_it_sits(gpu_ctx, shapes):
    probs = eu.batch_problems(shapes["mixed_70"], 21)
    S = [len(p["upstream"]) for p in probs]
    who = int(np.argmax([s if s <= 12 else 0 for s in S]))   # a path of several segments
    one = probs[who]
    rest = probs[:who] + probs[who + 1:]
    rows = []
    for at in (0, len(rest) // 2, len(rest)):
        batch = rest[:at] + [one] + rest[at:]
        so, wp, lim, g = eu.pack(batch)
        out = _backward(gpu_ctx, so, wp, lim, g)
        a, b = int(so[at]), int(so[at + 1])
        rows.append((out["term"][a:b], out["grad_waypoints"][a + at:b + at + 1], out["grad_limits"][at]))
    for r in rows[1:]:
        assert np.array_equal(r[0], rows[0][0]) and eu.same_bits(r[1], rows[0][1]) and eu.same_bits(r[2], rows[0][2])
    assert np.any(rows[0][1] != 0.0) and np.any(rows[0][2] != 0.0)


def test_zero_upstream_gives_exact_zero_rows_and_unread_limits_stay_zero(gpu_ctx, shapes):
    probs = eu.batch_problems(shapes["mixed_70"], 22)
    so, wp, lim, g = eu.pack(probs)
    dead = [3, 17, 40]   # paths whose whole upstream is zero, and NaN-free inputs all the same
    for q in dead:
        g[so[q]:so[q + 1]] = 0.0
    g[so[5]] = 0.0   # and one segment of a live path
    out = _backward(gpu_ctx, so, wp, lim, g)
    ref = _backward(gpu_ctx, so, wp, lim, g)
    for q in dead:
        assert np.all(eu.bits(out["grad_waypoints"][so[q] + q:so[q + 1] + q + 1]) == 0), q   # +0.0, every entry
        assert np.all(eu.bits(out["grad_limits"][q]) == 0), q
    assert np.all(out["grad_waypoints"][so[5] + 5] == 0.0)   # the first vertex of path 5 has that segment alone
    assert np.all(out["grad_limits"][:, list(eu.UNREAD_LIMITS)] == 0.0)
    assert np.any(out["grad_limits"][:, list(eu.READ_LIMITS)] != 0.0)
    for k in out:
        assert out[k].tobytes() == ref[k].tobytes(), k   # two calls, the same bits
    # the terms alone need no upstream and are the same
    assert np.array_equal(_backward(gpu_ctx, so, wp, lim, None, want=("term",))["term"], out["term"])
    # a waypoint that is not a number spoils its two segments and nothing else
    bad = wp.copy()
    v = int(so[8]) + 8 + 1   # the second vertex of path 8
    assert so[9] - so[8] >= 2
    bad[v, 0] = float("nan")
    nan = _backward(gpu_ctx, so, bad, lim, g)
    assert nan["term"][so[8]:so[8] + 2].tolist() == [eu.FLOOR, eu.FLOOR]
    assert np.all(np.isfinite(nan["grad_waypoints"])) and np.all(np.isfinite(nan["grad_limits"]))
    assert np.all(nan["grad_waypoints"][v] == 0.0)
    keep = np.ones(len(wp), dtype=bool)
    keep[v - 1:v + 2] = False
    assert eu.same_bits(nan["grad_waypoints"][keep], out["grad_waypoints"][keep])


def test_argument_errors(gpu_ctx, shapes):
    batch = shapes["uniform_70x3"]
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        wp, lim = _dev(batch.waypoints), _dev(batch.limits)
        g = torch.zeros(plan.n_segments, dtype=torch.float64, device="cuda")
        gw, gl = torch.zeros_like(wp), torch.zeros_like(lim)
        with pytest.raises(api.MrsTgError, match="every output"):
            plan.estimate_times_vjp(wp, lim, g)
        with pytest.raises(api.MrsTgError, match="need grad_seg_times"):
            plan.estimate_times_vjp(wp, lim, None, grad_waypoints=gw)
        with pytest.raises(api.MrsTgError, match="need grad_seg_times"):
            plan.estimate_times_vjp(wp, lim, None, grad_limits=gl, term=torch.zeros(plan.n_segments, dtype=torch.int32,
                                                                                    device="cuda"))
        with pytest.raises(api.MrsTgError):
            plan.estimate_times_vjp(None, lim, g, grad_waypoints=gw)
        with pytest.raises(api.MrsTgError):
            plan.estimate_times(wp, lim, None)
        with pytest.raises(ValueError):
            autograd.estimate_times(plan, wp[:-1], lim)
    finally:
        plan.close()


def _terms(plan, wp, lim):
    term = torch.empty(plan.n_segments, dtype=torch.int32, device="cuda")
    plan.estimate_times_vjp(wp, lim, term=term)
    return term


def _times(plan, wp, lim):
    t = torch.empty(plan.n_segments, dtype=torch.float64, device="cuda")
    plan.estimate_times(wp, lim, t)
    return t


def test_autograd_against_central_differences_of_the_gpu_forward(gpu_ctx, shapes):
    """Central differences with h = 1e-6 in every waypoint coordinate and in limits 0, 1, 2 and 5.  A segment reads two
    vertices that are neighbours in the array, so stepping one coordinate of every even (then every odd) vertex at once moves
    exactly one end of every segment: sixteen forward calls give every dt_i/ds and dt_i/de, eight more every dt_i/dlimit.  A
    segment whose term differs at any of the stepped points is left out of both sides (its upstream entry is zero); at most 5 %
    may be.  Agreement: 1e-7 of the largest gradient entry -- the forward's 1e-16 rounding over 2 h with a hundredfold margin."""
    batch = shapes["mixed_70"]
    h = 1e-6
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P, nS = batch.n_paths, batch.n_segments
    path_of_seg = np.repeat(np.arange(P), np.diff(so))
    start = np.arange(nS) + path_of_seg   # the vertex a segment starts at
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        gpu_ctx.use_torch_stream()
        wp0, lim0 = _dev(batch.waypoints), _dev(batch.limits)
        term0 = _terms(plan, wp0, lim0)
        same = torch.ones(nS, dtype=torch.bool, device="cuda")
        d_start, d_end = np.zeros((nS, 4)), np.zeros((nS, 4))
        parity = torch.arange(wp0.shape[0], device="cuda") % 2
        for k in range(4):
            for par in (0, 1):
                step = torch.zeros_like(wp0)
                step[:, k] = (parity == par).to(torch.float64) * h
                up, dn = wp0 + step, wp0 - step
                same &= (_terms(plan, up, lim0) == term0) & (_terms(plan, dn, lim0) == term0)
                width = ((up - wp0) + (wp0 - dn))[:, k].cpu().numpy()   # what the step really was, vertex by vertex
                diff = (_times(plan, up, lim0) - _times(plan, dn, lim0)).cpu().numpy()
                at_start = start % 2 == par
                d_start[at_start, k] = diff[at_start] / width[start[at_start]]
                d_end[~at_start, k] = diff[~at_start] / width[start[~at_start] + 1]
        d_lim = np.zeros((nS, 9))
        for k in eu.READ_LIMITS:
            step = torch.zeros_like(lim0)
            step[:, k] = h
            up, dn = lim0 + step, lim0 - step
            same &= (_terms(plan, wp0, up) == term0) & (_terms(plan, wp0, dn) == term0)
            width = ((up - lim0) + (lim0 - dn))[:, k].cpu().numpy()
            d_lim[:, k] = (_times(plan, wp0, up) - _times(plan, wp0, dn)).cpu().numpy() / width[path_of_seg]
        left_out = int((~same).sum())
        assert left_out <= 0.05 * nS, left_out
        g = _dev(eu.dyadic(np.random.default_rng(31), nS)) * same
        wp, lim = wp0.clone().requires_grad_(True), lim0.clone().requires_grad_(True)
        times = autograd.estimate_times(plan, wp, lim)
        assert eu.same_bits(times.detach().cpu().numpy(), _times(plan, wp0, lim0).cpu().numpy())
        (times * g).sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.close()
    gh = g.cpu().numpy()
    fd_w = np.zeros((nS + P, 4))
    np.add.at(fd_w, start, gh[:, None] * d_start)
    np.add.at(fd_w, start + 1, gh[:, None] * d_end)
    fd_l = np.zeros((P, 9))
    np.add.at(fd_l, path_of_seg, gh[:, None] * d_lim)
    gw, gl = wp.grad.cpu().numpy(), lim.grad.cpu().numpy()
    ew, el = np.abs(gw - fd_w).max(), np.abs(gl - fd_l).max()
    print("ESTIMATE GPU CENTRAL DIFFERENCES: %d of %d segments left out; waypoints max |diff| %.2e of max |grad| %.2e; limits "
          "%.2e of %.2e" % (left_out, nS, ew, np.abs(gw).max(), el, np.abs(gl).max()))
    assert np.abs(gw).max() > 0.1 and np.abs(gl).max() > 0.1
    assert ew <= 1e-7 * np.abs(gw).max() and el <= 1e-7 * np.abs(gl).max()


@pytest.mark.parametrize("scaled", [False, True])
def test_the_chain_from_the_waypoints_is_wired_bit_for_bit(gpu_ctx, scaled):
    """estimate_times -> solve [-> scale_times_to_limits -> solve] -> sample -> path_deviation -> corridor loss, once with the
    times from autograd.estimate_times and once with the same times as a leaf.  No tolerance: waypoints.grad of the first run
    is the second run's fixed_values.grad[:, 0, :] plus its path_deviation waypoint gradient plus
    Plan.estimate_times_vjp(times.grad), and limits.grad is the second run's plus the same call's limit gradient.  (Three
    addends have three sums; the autograd engine adds them as the backward nodes finish, which is its business: any of the
    three roundings is accepted, nothing else.)"""
    batch = du.chain_batch()
    cap, dt, corridor = du.CHAIN_CAPACITY, du.CHAIN_DT, du.CHAIN_CORRIDOR
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    try:
        def tail(fv, wp, lim, times):
            coeffs, _, status = autograd.solve(plan, mask, fv, times)
            if scaled:
                times = autograd.scale_times_to_limits(plan, coeffs, times, lim, status)
                coeffs, _, status = autograd.solve(plan, mask, fv, times)
            samples, n = autograd.sample(plan, coeffs, times, dt, cap, status)
            d, _ = autograd.path_deviation(plan, samples, n, wp, first_segment=True, status=status)
            assert bool(torch.all(status > 0))
            return torch.relu(d - corridor).sum()

        # first run: everything hangs on the waypoints and the limits
        wp1, lim1 = _dev(batch.waypoints).requires_grad_(True), _dev(batch.limits).requires_grad_(True)
        fv1 = _dev(batch.fixed_values).clone()
        fv1[:, 0, :] = wp1
        times1 = autograd.estimate_times(plan, wp1, lim1)
        times1.retain_grad()
        loss1 = tail(fv1, wp1, lim1, times1)
        loss1.backward()
        # second run: the same times as a leaf, the three ways to the waypoints kept apart
        fv2 = fv1.detach().clone().requires_grad_(True)
        wp2, lim2 = _dev(batch.waypoints).requires_grad_(True), _dev(batch.limits).requires_grad_(True)
        times2 = times1.detach().clone().requires_grad_(True)
        loss2 = tail(fv2, wp2, lim2, times2)
        loss2.backward()
        gw = torch.empty_like(wp2)
        gl = torch.empty_like(lim2)
        gpu_ctx.use_torch_stream()
        plan.estimate_times_vjp(wp2.detach(), lim2.detach(), times2.grad, grad_waypoints=gw, grad_limits=gl)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert eu.same_bits(loss1.detach().cpu().numpy(), loss2.detach().cpu().numpy()) and float(loss1.detach()) > 0
    assert eu.same_bits(times1.grad.cpu().numpy(), times2.grad.cpu().numpy()) and bool(torch.any(times2.grad != 0))
    a, b, c = fv2.grad[:, 0, :], wp2.grad, gw
    assert bool(torch.any(a != 0)) and bool(torch.any(b != 0)) and bool(torch.any(c != 0))
    got = wp1.grad.cpu().numpy()
    sums = [((x + y) + z).cpu().numpy() for x, y, z in ((a, b, c), (a, c, b), (b, c, a))]
    assert any(eu.same_bits(got, s) for s in sums), [float(np.abs(got - s).max()) for s in sums]
    direct = torch.zeros_like(gl) if lim2.grad is None else lim2.grad
    assert (lim2.grad is not None) == scaled
    assert eu.same_bits(lim1.grad.cpu().numpy(), (direct + gl).cpu().numpy())
    assert bool(torch.any(gl != 0))

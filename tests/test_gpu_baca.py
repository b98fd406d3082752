"""mrs_tg_plan_estimate_times_baca / mrs_tg_plan_estimate_times_baca_vjp / mrs_tg_plan_length_gate on the GPU (baca_times_kernel,
baca_times_vjp_kernel, length_gate_kernel) and autograd.estimate_times_baca on top of them: the forward
against the oracle, the library's host estimate and the 60-digit fixtures, the backward pass against the fixtures, against the
CPU harness bit for bit and against central differences of the GPU forward, and the gate against the host's sums and a
restatement of length_check.  NaN inputs are ordinary data here: nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from oracle import pyoracle as po
from tests import baca_util as bu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
SHAPES = ["uniform_3x1", "uniform_70x3", "mixed_70", "one_path"]


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return bu.build_harness(tmp_path_factory.mktemp("baca_gpu"))


@pytest.fixture(scope="module")
def groups():
    """the fixture's paths and the four batches, as harness problems (dyadic upstreams)"""
    out = dict(fixture=[bu.case_problem(c) for c in bu.load_cases()])
    for n, (name, batch) in enumerate(bu.shapes().items()):
        out[name] = bu.batch_problems(batch, 10 + n)
    return out


@pytest.fixture(scope="module")
def cpu(harness, groups):
    """the harness's results for every group, computed once"""
    return {name: bu.run_harness(harness, probs) for name, probs in groups.items()}


def _guarded(rows, tail, dtype, fill):
    """a tensor with one guard row in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _unguard(full, fill, name):
    host = full.cpu().numpy()
    assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
    assert not np.any(host[1:-1] == fill), "%s: an element of the plan was not written" % name
    return host[1:-1].copy()


def _forward(ctx, so, wp, lim):
    plan = api.Plan(ctx, so)
    try:
        full, view = _guarded(int(so[-1]), (), torch.float64, SENTINEL)
        plan.estimate_times_baca(_dev(wp), _dev(lim), view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return _unguard(full, SENTINEL, "seg_times")


def _backward(ctx, so, wp, lim, upstream, want=("grad_waypoints", "grad_limits", "flags")):
    """one backward call -> host arrays by name; every output is prefilled with a sentinel and has guard rows on both sides"""
    P, nS = len(so) - 1, int(so[-1])
    spec = dict(grad_waypoints=(nS + P, (4,), torch.float64, SENTINEL), grad_limits=(P, (9,), torch.float64, SENTINEL),
                flags=(nS, (), torch.int32, ISENTINEL))
    full, view = {}, {}
    for name in want:
        full[name], view[name] = _guarded(*spec[name])
    plan = api.Plan(ctx, so)
    try:
        plan.estimate_times_baca_vjp(_dev(wp), _dev(lim), None if upstream is None else _dev(upstream), **view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return {name: _unguard(full[name], spec[name][3], name) for name in want}


def _gate(ctx, so, times, n_samples, dt, max_factor, min_factor, status, want=("total", "verdict")):
    P = len(so) - 1
    spec = dict(total=(P, (), torch.float64, SENTINEL), verdict=(P, (), torch.int32, ISENTINEL))
    full, view = {}, {}
    for name in want:
        full[name], view[name] = _guarded(*spec[name])
    plan = api.Plan(ctx, so)
    try:
        plan.length_gate(_dev(times), _dev(n_samples, np.int32), dt, max_factor, min_factor,
                         status=None if status is None else _dev(status, np.int32), **view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return {name: _unguard(full[name], spec[name][3], name) for name in want}


def _compare_with_harness(out, cpu_results, so):
    for q, h in enumerate(cpu_results):
        a, b = int(so[q]), int(so[q + 1])
        assert np.array_equal(out["flags"][a:b], h["flags"]), q
        assert bu.same_bits(out["grad_waypoints"][a + q:b + q + 1], h["grad_waypoints"]), q
        assert bu.same_bits(out["grad_limits"][q], h["grad_limits"]), q


def test_the_library_reports_the_capability_and_times_the_three_kernels(gpu_ctx, groups):
    assert api.CAP_BACA == 1024 and api.capabilities() & api.CAP_BACA
    assert (api.BACA_V_VERTICAL, api.BACA_A_VERTICAL, api.BACA_J_VERTICAL, api.BACA_T1_CAPPED, api.BACA_T2_CAPPED,
            api.BACA_DOT1_CLAMPED, api.BACA_DOT2_CLAMPED, api.BACA_FLOOR, api.BACA_HEADING, api.BACA_HEADING_CRUISE,
            api.BACA_HEADING_ACC) == (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) == \
        (bu.V_VERTICAL, bu.A_VERTICAL, bu.J_VERTICAL, bu.T1_CAPPED, bu.T2_CAPPED, bu.DOT1_CLAMPED, bu.DOT2_CLAMPED, bu.FLOOR,
         bu.HEADING, bu.HEADING_CRUISE, bu.HEADING_ACC)
    assert (api.KERNEL_BACA, api.KERNEL_BACA_VJP, api.KERNEL_LENGTH_GATE) == (14, 15, 16)
    assert (api.FIND_ACCEPTED, api.FIND_REJECTED_CODE, api.FIND_REJECTED_TOO_LONG, api.FIND_REJECTED_TOO_SHORT) == \
        (bu.ACCEPTED, bu.REJECTED_CODE, bu.TOO_LONG, bu.TOO_SHORT)
    so, wp, lim, g = bu.pack(groups["uniform_70x3"])
    try:
        gpu_ctx.set_profiling(True)
        times = _forward(gpu_ctx, so, wp, lim)
        _backward(gpu_ctx, so, wp, lim, g)
        _gate(gpu_ctx, so, times, np.full(len(so) - 1, 40), 0.2, 3.0, 0.33, None)
        for kernel in (api.KERNEL_BACA, api.KERNEL_BACA_VJP, api.KERNEL_LENGTH_GATE):
            assert gpu_ctx.last_kernel_ms(kernel) > 0, kernel
    finally:
        gpu_ctx.set_profiling(False)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_within_1e_13_of_the_oracle_and_of_the_host_estimate(gpu_ctx, groups, shape):
    probs = groups[shape]
    so, wp, lim, _ = bu.pack(probs)
    times = _forward(gpu_ctx, so, wp, lim)
    worst = 0.0
    for q, p in enumerate(probs):
        got = times[so[q]:so[q + 1]]
        ref = po.estimate_times(p["waypoints"], p["limits"], baca=True)
        host = api.estimate_times_baca(p["waypoints"], p["limits"])
        worst = max(worst, float(np.max(np.abs(got - ref) / ref)), float(np.max(np.abs(got - host) / host)))
        assert np.all(np.abs(got - ref) <= bu.VALUE_RTOL * ref), q
        assert np.all(np.abs(got - host) <= bu.VALUE_RTOL * host), q
    print("BACA GPU FORWARD %s: worst relative difference %.2e" % (shape, worst))


def test_fixture_through_the_gpu(gpu_ctx, groups):
    cases = bu.load_cases()
    so, wp, lim, g = bu.pack(groups["fixture"])
    times = _forward(gpu_ctx, so, wp, lim)
    out = _backward(gpu_ctx, so, wp, lim, g)
    report, worst = {}, 0.0
    for q, c in enumerate(cases):
        a, b = int(so[q]), int(so[q + 1])
        assert out["flags"][a:b].tolist() == c["flags"], c["name"]
        exact = np.array(c["value"])
        worst = max(worst, float(np.max(np.abs(times[a:b] - exact) / exact)))
        assert np.all(np.abs(times[a:b] - exact) <= bu.VALUE_RTOL * exact), c["name"]
        floor = (np.array(c["flags"]) & (bu.FLOOR | bu.HEADING)) == bu.FLOOR
        assert np.all(times[a:b][floor] == 0.01), c["name"]
        ew, el, ratio = bu.gradient_excess(c, out["grad_waypoints"][a + q:b + q + 1], out["grad_limits"][q])
        report[c["name"]] = "%.3f" % ratio
        assert ew <= 0.0 and el <= 0.0, (c["name"], ew, el)
    print("BACA GPU FIXTURE VALUES: worst relative error %.2e" % worst)
    print("BACA GPU GRADIENT FIXTURES, largest |error| / bound: %s" % report)


@pytest.mark.parametrize("group", ["fixture"] + SHAPES)
def test_gpu_gradients_and_flags_are_the_harness_in_bits(gpu_ctx, groups, cpu, group):
    so, wp, lim, g = bu.pack(groups[group])
    out = _backward(gpu_ctx, so, wp, lim, g)
    _compare_with_harness(out, cpu[group], so)
    assert np.all(out["grad_limits"][:, 8] == 0.0)
    if group == "mixed_70":
        S = np.diff(so)
        assert int(so[-1]) + len(S) > 256 and S.min() == 1 and S.max() > 25 and len(set(S.tolist())) > 10
        seen = int(np.bitwise_or.reduce(out["flags"]))
        assert seen & 7 and seen & 24 and seen & 96 and seen & bu.HEADING, seen
        only = _backward(gpu_ctx, so, wp, lim, None, want=("flags",))   # the flags alone need no upstream and are the same
        assert np.array_equal(only["flags"], out["flags"])
        assert np.any(out["grad_waypoints"] != 0.0) and np.any(out["grad_limits"] != 0.0)


def test_a_path_gives_the_same_bits_wherever_it_sits(gpu_ctx, groups):
    """the mixed batch reversed, and one path of it alone: the forward and the backward of every path in the same bits -- a
    neighbour read across a path edge would show here"""
    probs = groups["mixed_70"]
    so, wp, lim, g = bu.pack(probs)
    times = _forward(gpu_ctx, so, wp, lim)
    out = _backward(gpu_ctx, so, wp, lim, g)
    rev = probs[::-1]
    so_r, wp_r, lim_r, g_r = bu.pack(rev)
    times_r = _forward(gpu_ctx, so_r, wp_r, lim_r)
    out_r = _backward(gpu_ctx, so_r, wp_r, lim_r, g_r)
    P = len(probs)
    for q in range(P):
        r = P - 1 - q
        a, b, ar, br = int(so[q]), int(so[q + 1]), int(so_r[r]), int(so_r[r + 1])
        assert bu.same_bits(times[a:b], times_r[ar:br]), q
        assert np.array_equal(out["flags"][a:b], out_r["flags"][ar:br]), q
        assert bu.same_bits(out["grad_waypoints"][a + q:b + q + 1], out_r["grad_waypoints"][ar + r:br + r + 1]), q
        assert bu.same_bits(out["grad_limits"][q], out_r["grad_limits"][r]), q
    who = int(np.argmax([len(p["upstream"]) if len(p["upstream"]) <= 12 else 0 for p in probs]))   # a path of several segments
    assert len(probs[who]["upstream"]) >= 4
    so_1, wp_1, lim_1, g_1 = bu.pack([probs[who]])
    a, b = int(so[who]), int(so[who + 1])
    assert bu.same_bits(_forward(gpu_ctx, so_1, wp_1, lim_1), times[a:b])
    alone = _backward(gpu_ctx, so_1, wp_1, lim_1, g_1)
    assert np.array_equal(alone["flags"], out["flags"][a:b])
    assert bu.same_bits(alone["grad_waypoints"], out["grad_waypoints"][a + who:b + who + 1])
    assert bu.same_bits(alone["grad_limits"][0], out["grad_limits"][who])
    assert np.any(alone["grad_waypoints"] != 0.0) and np.any(alone["grad_limits"] != 0.0)


def test_exact_zero_rows(gpu_ctx, groups):
    probs = groups["mixed_70"]
    so, wp, lim, g = bu.pack(probs)
    g = g.copy()
    dead = [3, 17, 40]   # paths whose whole upstream is zero
    for q in dead:
        g[so[q]:so[q + 1]] = 0.0
    out = _backward(gpu_ctx, so, wp, lim, g)
    ref = _backward(gpu_ctx, so, wp, lim, g)
    for q in dead:
        assert np.all(bu.bits(out["grad_waypoints"][so[q] + q:so[q + 1] + q + 1]) == 0), q   # +0.0, every entry
        assert np.all(bu.bits(out["grad_limits"][q]) == 0), q
    assert np.all(bu.bits(out["grad_limits"][:, 8]) == 0)   # entry 8, every path
    for k in out:
        assert out[k].tobytes() == ref[k].tobytes(), k   # two calls, the same bits
    # a waypoint that is not a number spoils the segments that read it and nothing else: FLOOR, zero rows
    q = next(q for q in range(len(probs)) if so[q + 1] - so[q] >= 7 and q not in dead)
    bad = wp.copy()
    v = int(so[q]) + q + 3   # the fourth vertex of that path: read by its segments 1 .. 4
    bad[v, 0] = float("nan")
    nan = _backward(gpu_ctx, so, bad, lim, g)
    assert nan["flags"][so[q] + 1:so[q] + 5].tolist() == [bu.FLOOR] * 4
    assert np.all(np.isfinite(nan["grad_waypoints"])) and np.all(np.isfinite(nan["grad_limits"]))
    quiet = g.copy()
    quiet[so[q] + 1:so[q] + 5] = 0.0
    same = _backward(gpu_ctx, so, wp, lim, quiet)
    assert bu.same_bits(nan["grad_waypoints"], same["grad_waypoints"]) and bu.same_bits(nan["grad_limits"], same["grad_limits"])
    keep = np.ones(int(so[-1]), dtype=bool)
    keep[so[q] + 1:so[q] + 5] = False
    assert np.array_equal(nan["flags"][keep], out["flags"][keep])
    # the forward of those segments is what the arithmetic gives (not a number), the others' in the same bits
    t_bad, t_ok = _forward(gpu_ctx, so, bad, lim), _forward(gpu_ctx, so, wp, lim)
    assert bu.same_bits(t_bad[keep], t_ok[keep])
    # FLOOR: the fixture's 5 mm segment alone gives zero rows
    c = next(c for c in bu.load_cases() if c["name"] == "five_millimetres")
    p = bu.case_problem(c)
    so_f, wp_f, lim_f, g_f = bu.pack([dict(p, upstream=p["upstream"] * np.array([0.0, 1.0, 0.0]))])
    floor = _backward(gpu_ctx, so_f, wp_f, lim_f, g_f)
    assert floor["flags"][1] & (bu.FLOOR | bu.HEADING) == bu.FLOOR
    assert np.all(bu.bits(floor["grad_waypoints"]) == 0) and np.all(bu.bits(floor["grad_limits"]) == 0)


def test_argument_errors(gpu_ctx, groups):
    so, wp_h, lim_h, _ = bu.pack(groups["uniform_70x3"])
    plan = api.Plan(gpu_ctx, so)
    try:
        wp, lim = _dev(wp_h), _dev(lim_h)
        g = torch.zeros(plan.n_segments, dtype=torch.float64, device="cuda")
        gw, gl = torch.zeros_like(wp), torch.zeros_like(lim)
        flags = torch.zeros(plan.n_segments, dtype=torch.int32, device="cuda")
        with pytest.raises(api.MrsTgError, match="every output"):
            plan.estimate_times_baca_vjp(wp, lim, g)
        with pytest.raises(api.MrsTgError, match="need grad_seg_times"):
            plan.estimate_times_baca_vjp(wp, lim, None, grad_waypoints=gw)
        with pytest.raises(api.MrsTgError, match="need grad_seg_times"):
            plan.estimate_times_baca_vjp(wp, lim, None, grad_limits=gl, flags=flags)
        with pytest.raises(api.MrsTgError):
            plan.estimate_times_baca_vjp(None, lim, g, grad_waypoints=gw)
        with pytest.raises(api.MrsTgError):
            plan.estimate_times_baca(wp, lim, None)
        n = torch.zeros(plan.n_paths, dtype=torch.int32, device="cuda")
        with pytest.raises(api.MrsTgError, match="both NULL"):
            plan.length_gate(g, n, 0.2)
        with pytest.raises(api.MrsTgError):
            plan.length_gate(None, n, 0.2, verdict=torch.zeros(plan.n_paths, dtype=torch.int32, device="cuda"))
        with pytest.raises(ValueError):
            autograd.estimate_times_baca(plan, wp[:-1], lim)
    finally:
        plan.close()


def _flags(plan, wp, lim):
    f = torch.empty(plan.n_segments, dtype=torch.int32, device="cuda")
    plan.estimate_times_baca_vjp(wp, lim, flags=f)
    return f


def _times(plan, wp, lim):
    t = torch.empty(plan.n_segments, dtype=torch.float64, device="cuda")
    plan.estimate_times_baca(wp, lim, t)
    return t


def test_autograd_against_central_differences_of_the_gpu_forward(gpu_ctx, groups):
    """Central differences with h = 1e-6 in every waypoint coordinate and in limits 0 .. 7.  A segment reads four vertices that
    are neighbours in the array (pre, start, end, post, of its own path), so stepping one coordinate of every fourth vertex at
    once moves exactly one of them for every segment: thirty-two forward calls give every dt_i/d(pre, s, e, post), sixteen more
    every dt_i/dlimit.  A segment whose flags differ at any of the stepped points is left out of both sides (its upstream
    entry is zero); at most 5 % may be.  Agreement: 1e-7 of the largest gradient entry (the figures of DESIGN.md section 4e)."""
    probs = groups["mixed_70"]
    so, wp_h, lim_h, _ = bu.pack(probs)
    h = 1e-6
    so64 = np.asarray(so, dtype=np.int64)
    P, nS = len(so) - 1, int(so[-1])
    path_of_seg = np.repeat(np.arange(P), np.diff(so64))
    start = np.arange(nS) + path_of_seg            # the vertex a segment starts at
    first, last = (so64[:-1] + np.arange(P))[path_of_seg], (so64[1:] + np.arange(P))[path_of_seg]   # its path's first / last vertex
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp0, lim0 = _dev(wp_h), _dev(lim_h)
        flags0 = _flags(plan, wp0, lim0)
        same = torch.ones(nS, dtype=torch.bool, device="cuda")
        fd_parts = []   # (vertex of every segment, coordinate, dt_i/d that coordinate)
        residue = torch.arange(wp0.shape[0], device="cuda") % 4
        for k in range(4):
            for r in range(4):
                step = torch.zeros_like(wp0)
                step[:, k] = (residue == r).to(torch.float64) * h
                up, dn = wp0 + step, wp0 - step
                same &= (_flags(plan, up, lim0) == flags0) & (_flags(plan, dn, lim0) == flags0)
                width = ((up - wp0) + (wp0 - dn))[:, k].cpu().numpy()   # what the step really was, vertex by vertex
                diff = (_times(plan, up, lim0) - _times(plan, dn, lim0)).cpu().numpy()
                v = start - 1 + ((r - (start - 1)) % 4)   # the one of start - 1 .. start + 2 with that residue
                inside = (v >= first) & (v <= last)
                assert np.all(diff[~inside] == 0.0)       # a vertex of another path moves nothing
                fd_parts.append((v[inside], k, diff[inside] / width[v[inside]], inside))
        d_lim = np.zeros((nS, 9))
        for k in range(8):
            step = torch.zeros_like(lim0)
            step[:, k] = h
            up, dn = lim0 + step, lim0 - step
            same &= (_flags(plan, wp0, up) == flags0) & (_flags(plan, wp0, dn) == flags0)
            width = ((up - lim0) + (lim0 - dn))[:, k].cpu().numpy()
            d_lim[:, k] = (_times(plan, wp0, up) - _times(plan, wp0, dn)).cpu().numpy() / width[path_of_seg]
        left_out = int((~same).sum())
        assert left_out <= 0.05 * nS, left_out
        g = _dev(bu.dyadic(np.random.default_rng(31), nS)) * same
        wp, lim = wp0.clone().requires_grad_(True), lim0.clone().requires_grad_(True)
        times = autograd.estimate_times_baca(plan, wp, lim)
        assert bu.same_bits(times.detach().cpu().numpy(), _times(plan, wp0, lim0).cpu().numpy())
        (times * g).sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.close()
    gh = g.cpu().numpy()
    fd_w = np.zeros((nS + P, 4))
    for v, k, d, inside in fd_parts:
        np.add.at(fd_w[:, k], v, gh[inside] * d)
    fd_l = np.zeros((P, 9))
    np.add.at(fd_l, path_of_seg, gh[:, None] * d_lim)
    gw, gl = wp.grad.cpu().numpy(), lim.grad.cpu().numpy()
    ew, el = np.abs(gw - fd_w).max(), np.abs(gl - fd_l).max()
    print("BACA GPU CENTRAL DIFFERENCES: %d of %d segments left out; waypoints max |diff| %.2e of max |grad| %.2e; limits "
          "%.2e of %.2e" % (left_out, nS, ew, np.abs(gw).max(), el, np.abs(gl).max()))
    assert np.abs(gw).max() > 0.1 and np.abs(gl).max() > 0.1
    assert ew <= 1e-7 * np.abs(gw).max() and el <= 1e-7 * np.abs(gl).max()


def test_autograd_is_wired_to_the_backward_call_bit_for_bit(gpu_ctx, groups):
    """waypoints.grad and limits.grad of sum_i w_i t_i are Plan.estimate_times_baca_vjp(w): no tolerance"""
    so, wp_h, lim_h, g_h = bu.pack(groups["mixed_70"])
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp, lim = _dev(wp_h).requires_grad_(True), _dev(lim_h).requires_grad_(True)
        weights = _dev(g_h)
        times = autograd.estimate_times_baca(plan, wp, lim)
        (times * weights).sum().backward()
        gw, gl = torch.empty_like(wp), torch.empty_like(lim)
        plan.estimate_times_baca_vjp(wp.detach(), lim.detach(), weights, grad_waypoints=gw, grad_limits=gl)
        torch.cuda.synchronize()
        assert bu.same_bits(times.detach().cpu().numpy(), _times(plan, wp.detach(), lim.detach()).cpu().numpy())
        # one input alone: the other gradient is not asked for
        wp2 = _dev(wp_h).requires_grad_(True)
        (autograd.estimate_times_baca(plan, wp2, _dev(lim_h)) * weights).sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert bu.same_bits(wp.grad.cpu().numpy(), gw.cpu().numpy()) and bu.same_bits(lim.grad.cpu().numpy(), gl.cpu().numpy())
    assert bu.same_bits(wp2.grad.cpu().numpy(), gw.cpu().numpy())
    assert bool(torch.any(gw != 0)) and bool(torch.any(gl != 0))


def _gate_inputs(probs, so):
    """the host's Baca times of every path, and per path a sample count at 0.2, 1 or 3.5 x total / dt (by turns), one path
    with n dt <= 1 and one with a code the nodelet rejects"""
    dt = 0.2
    times = np.concatenate([api.estimate_times_baca(p["waypoints"], p["limits"]) for p in probs])
    P = len(probs)
    n = np.zeros(P, dtype=np.int32)
    status = np.ones(P, dtype=np.int32)
    for q in range(P):
        total = bu.gate_restatement(times[so[q]:so[q + 1]], 0, dt, 0, 0)[0]
        n[q] = int((0.2, 1.0, 3.5)[q % 3] * total / dt)
    n[4] = 5                                   # 1.0 s: not longer than one second
    status[7] = 6                              # MAXTIME, with a count that would be too long
    n[7] = max(n[7], int(3.5 * bu.gate_restatement(times[so[7]:so[7 + 1]], 0, dt, 0, 0)[0] / dt))
    status[10], status[11] = -1, 4             # accepted codes
    return times, n, status, dt


def test_the_gate_on_the_hosts_times_is_the_hosts_sum_and_length_check(gpu_ctx, groups):
    probs = groups["mixed_70"]
    so = bu.pack(probs)[0]
    times, n, status, dt = _gate_inputs(probs, so)
    P = len(probs)
    for max_factor, min_factor, with_status in ((3.0, 0.33, True), (3.0, 0.33, False), (0.0, 0.33, True), (3.0, -1.0, True)):
        out = _gate(gpu_ctx, so, times, n, dt, max_factor, min_factor, status if with_status else None)
        want = [bu.gate_restatement(times[so[q]:so[q + 1]], int(n[q]), dt, max_factor, min_factor, int(status[q]) if with_status else None)
                for q in range(P)]
        assert bu.same_bits(out["total"], np.array([t for t, _ in want]))     # the host's sequential sums, in bits
        assert out["verdict"].tolist() == [v for _, v in want]
        if (max_factor, min_factor, with_status) == (3.0, 0.33, True):
            assert set(out["verdict"].tolist()) == {bu.ACCEPTED, bu.REJECTED_CODE, bu.TOO_LONG, bu.TOO_SHORT}
            assert out["verdict"][4] == bu.ACCEPTED and out["verdict"][7] == bu.REJECTED_CODE
            first = out
        if max_factor == 0.0:
            assert bu.TOO_LONG not in out["verdict"].tolist() and bu.TOO_SHORT in out["verdict"].tolist()
        if min_factor < 0:
            assert bu.TOO_SHORT not in out["verdict"].tolist() and bu.TOO_LONG in out["verdict"].tolist()
        if not with_status:
            assert out["verdict"][7] == bu.TOO_LONG
    # either output alone
    assert np.array_equal(_gate(gpu_ctx, so, times, n, dt, 3.0, 0.33, status, want=("verdict",))["verdict"], first["verdict"])
    assert bu.same_bits(_gate(gpu_ctx, so, times, n, dt, 3.0, 0.33, status, want=("total",))["total"], first["total"])
    # the order of the sum is observable on some path
    assert any(not bu.same_bits(first["total"][q], bu.gate_restatement(times[so[q]:so[q + 1]][::-1], 0, dt, 0, 0)[0]) for q in range(P))


def test_the_gate_on_the_devices_times_gives_the_same_verdicts(gpu_ctx, groups):
    probs = groups["mixed_70"]
    so, wp, lim, _ = bu.pack(probs)
    times, n, status, dt = _gate_inputs(probs, so)
    host = _gate(gpu_ctx, so, times, n, dt, 3.0, 0.33, status)
    plan = api.Plan(gpu_ctx, so)
    try:   # estimate and gate on the device, nothing comes down in between
        t = torch.empty(plan.n_segments, dtype=torch.float64, device="cuda")
        plan.estimate_times_baca(_dev(wp), _dev(lim), t)
        total = torch.empty(plan.n_paths, dtype=torch.float64, device="cuda")
        verdict = torch.empty(plan.n_paths, dtype=torch.int32, device="cuda")
        plan.length_gate(t, _dev(n, np.int32), dt, 3.0, 0.33, status=_dev(status, np.int32), total=total, verdict=verdict)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert verdict.cpu().numpy().tolist() == host["verdict"].tolist()
    assert np.all(np.abs(total.cpu().numpy() - host["total"]) <= bu.VALUE_RTOL * host["total"])
    assert set(host["verdict"].tolist()) == {bu.ACCEPTED, bu.REJECTED_CODE, bu.TOO_LONG, bu.TOO_SHORT}

"""mrs_tg_plan_unwrap_headings / mrs_tg_plan_fallback_sample / mrs_tg_plan_fallback_sample_vjp on the GPU (unwrap_headings_kernel,
fallback_sample_kernel, fallback_sample_vjp_kernel) and autograd.fallback_sample / fallback_trajectory on
top of them: counts, first rows and x, y, z against the CPU harness bit for bit, headings within the counted bound of
tests/fallback_util.py, the whole chain against the oracle's mto_fallback_sampling, the backward pass against the harness bit for
bit and against central differences of the GPU forward.  NaN and inf times are ordinary data here: nothing provokes a fault."""
import math

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import fallback_util as fu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
SHAPES = ["uniform_3x1", "uniform_70x3", "mixed_70", "one_path"]
INVALID_ARG = -1


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fu.build_harness(tmp_path_factory.mktemp("fallback_gpu"))


@pytest.fixture(scope="module")
def groups():
    """the four batches as explicit-time problems with dyadic upstreams (one dt, stopping time and capacity per batch)"""
    return {name: fu.batch_problems(batch, 10 + n) for n, (name, batch) in enumerate(fu.shapes().items())}


@pytest.fixture(scope="module")
def edge():
    """the edge cases, each with a dyadic upstream whose rows from min(count, capacity) on are NaN"""
    out = []
    for n, p in enumerate(fu.edge_cases()):
        ref = fu.reference_loop(p)
        up = fu.bu.dyadic(np.random.default_rng(800 + n), p["capacity"] * 4).reshape(p["capacity"], 4)
        up[min(ref["count"], p["capacity"]):] = np.nan
        out.append(dict(p, upstream=up))
    return out


@pytest.fixture(scope="module")
def cpu(harness, groups, edge):
    """the harness's results for every group, computed once"""
    out = {name: fu.run_harness(harness, probs) for name, probs in groups.items()}
    out["edge"] = fu.run_harness(harness, edge)
    return out


def _guarded(rows, tail, dtype, fill):
    """a tensor with one guard row in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _guards_untouched(full, fill, name):
    host = full.cpu().numpy()
    assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
    return host[1:-1].copy()


def _forward(ctx, probs):
    """one forward call on the problems as a batch -> (n_samples [P], samples [P][cap][4] with the sentinel where nothing was
    written, seg_first_row [sum S]); every output prefilled with a sentinel, guard rows on both sides"""
    so, wp, stop, times, _ = fu.pack(probs)
    P, cap, p0 = len(probs), probs[0]["capacity"], probs[0]
    n_full, n_view = _guarded(P, (), torch.int32, ISENTINEL)
    s_full, s_view = _guarded(P, (cap, 4), torch.float64, SENTINEL)
    f_full, f_view = _guarded(int(so[-1]), (), torch.int32, ISENTINEL)
    plan = api.Plan(ctx, so)
    try:
        ctx.use_torch_stream()
        plan.fallback_sample(_dev(wp), _dev(times), p0["dt"], cap, n_view, s_view, stop_at=_dev(stop),
                             stopping_time=p0["stopping_time"], seg_first_row=f_view)
        torch.cuda.synchronize()
    finally:
        plan.close()
    n = _guards_untouched(n_full, ISENTINEL, "n_samples")
    first = _guards_untouched(f_full, ISENTINEL, "seg_first_row")
    samples = _guards_untouched(s_full, SENTINEL, "samples")
    assert not np.any(n == ISENTINEL) and not np.any(first == ISENTINEL)
    for q in range(P):
        k = min(int(n[q]), cap)
        assert not np.any(samples[q, :k] == SENTINEL), "path %d: a row below n was not written" % q
        assert np.all(samples[q, k:] == SENTINEL), "path %d: a row from n on was written" % q
    return n, samples, first, so


def _backward(ctx, probs, upstream=None):
    so, _, stop, times, up = fu.pack(probs)
    p0 = probs[0]
    g_full, g_view = _guarded(int(so[-1]) + len(probs), (4,), torch.float64, SENTINEL)
    plan = api.Plan(ctx, so)
    try:
        ctx.use_torch_stream()
        plan.fallback_sample_vjp(_dev(times), p0["dt"], p0["capacity"], _dev(up if upstream is None else upstream), g_view,
                                 stop_at=_dev(stop), stopping_time=p0["stopping_time"])
        torch.cuda.synchronize()
    finally:
        plan.close()
    g = _guards_untouched(g_full, SENTINEL, "grad_waypoints")
    assert not np.any(g == SENTINEL), "an element of the plan was not written"
    return g, so


def _compare_forward(n, samples, first, so, cpu_results, cap):
    """counts, first rows, x, y, z in bits; headings within the bound -> the worst heading difference"""
    worst = 0.0
    for q, h in enumerate(cpu_results):
        a, b = int(so[q]), int(so[q + 1])
        assert int(n[q]) == h["n_samples"], (q, int(n[q]), h["n_samples"])
        assert np.array_equal(first[a:b], h["seg_first_row"]), q
        k = min(h["n_samples"], cap)
        assert fu.same_bits(samples[q, :k, :3], h["rows"][:, :3]), q
        if k:
            d = fu.wrapped_difference(samples[q, :k, 3], h["rows"][:, 3])
            worst = max(worst, float(d.max()))
            assert np.all(d <= fu.HEADING_BOUND), (q, float(d.max()), fu.HEADING_BOUND)
            assert np.all(np.abs(samples[q, :k, 3]) <= math.pi)
    return worst


def test_the_library_reports_the_capability_and_times_the_three_kernels(gpu_ctx, groups):
    assert api.CAP_FALLBACK_SAMPLE == 2048 and api.capabilities() & api.CAP_FALLBACK_SAMPLE
    assert (api.KERNEL_UNWRAP_HEADINGS, api.KERNEL_FALLBACK_SAMPLE, api.KERNEL_FALLBACK_SAMPLE_VJP) == (17, 18, 19)
    lib = api.load_library()
    for name in ("mrs_tg_plan_unwrap_headings", "mrs_tg_plan_fallback_sample", "mrs_tg_plan_fallback_sample_vjp"):
        assert hasattr(lib, name) and name in api.EXPORTED_SYMBOLS
    assert lib.mrs_tg_abi_version() == 5
    probs = groups["uniform_70x3"]
    so, wp, _, _, _ = fu.pack(probs)
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        _forward(gpu_ctx, probs)
        _backward(gpu_ctx, probs)
        plan = api.Plan(gpu_ctx, so)
        try:
            plan.unwrap_headings(_dev(wp))
            torch.cuda.synchronize()
        finally:
            plan.close()
        mine = ("fallback_sample_kernel", "fallback_sample_vjp_kernel", "unwrap_headings_kernel")
        assert tuple(k for k in api.kernel_trace() if k in mine) == mine, api.kernel_trace()
        for kernel in (api.KERNEL_UNWRAP_HEADINGS, api.KERNEL_FALLBACK_SAMPLE, api.KERNEL_FALLBACK_SAMPLE_VJP):
            assert gpu_ctx.last_kernel_ms(kernel) > 0, kernel
    finally:
        gpu_ctx.set_profiling(False)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_is_the_harness(gpu_ctx, groups, cpu, shape):
    probs = groups[shape]
    n, samples, first, so = _forward(gpu_ctx, probs)
    worst = _compare_forward(n, samples, first, so, cpu[shape], probs[0]["capacity"])
    print("FALLBACK GPU FORWARD %s: worst heading difference %.3e = %.3f of the bound %.3e"
          % (shape, worst, worst / fu.HEADING_BOUND, fu.HEADING_BOUND))
    if shape == "mixed_70":
        counts = np.array([h["count"] for h in cpu[shape]])
        cap = probs[0]["capacity"]
        assert np.any(counts > cap) and np.any(counts < cap) and np.any(first == cap + 1)   # paths that overrun and that fit
        assert sum(int(p["stop_at"][1:-1].sum()) for p in probs) > 50


def test_edge_cases_through_the_gpu(gpu_ctx, edge, cpu):
    worst = 0.0
    for p, h in zip(edge, cpu["edge"]):
        n, samples, first, so = _forward(gpu_ctx, [p])
        worst = max(worst, _compare_forward(n, samples, first, so, [h], p["capacity"]))
        g, _ = _backward(gpu_ctx, [p])
        assert fu.same_bits(g, h["grad_waypoints"]), p["name"]      # (finite: the NaN rows from n on were never read)
    print("FALLBACK GPU EDGE CASES: worst heading difference %.3e = %.3f of the bound" % (worst, worst / fu.HEADING_BOUND))


def test_no_stop_at_pointer_is_nobody_stops(gpu_ctx, groups, harness):
    probs = [dict(p, stop_at=np.zeros_like(p["stop_at"])) for p in groups["uniform_70x3"]]
    ref = fu.run_harness(harness, probs)
    so, wp, _, times, up = fu.pack(probs)
    cap, p0 = probs[0]["capacity"], probs[0]
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        n = torch.full((len(probs),), ISENTINEL, dtype=torch.int32, device="cuda")
        s = torch.full((len(probs), cap, 4), SENTINEL, dtype=torch.float64, device="cuda")
        plan.fallback_sample(_dev(wp), _dev(times), p0["dt"], cap, n, s)     # no stop_at, no seg_first_row
        g = torch.full((int(so[-1]) + len(probs), 4), SENTINEL, dtype=torch.float64, device="cuda")
        plan.fallback_sample_vjp(_dev(times), p0["dt"], cap, _dev(up), g)
        torch.cuda.synchronize()
    finally:
        plan.close()
    n, s, g = n.cpu().numpy(), s.cpu().numpy(), g.cpu().numpy()
    for q, h in enumerate(ref):
        assert int(n[q]) == h["n_samples"] and fu.same_bits(s[q, :min(h["n_samples"], cap), :3], h["rows"][:, :3]), q
        assert fu.same_bits(g[so[q] + q:so[q + 1] + q + 1], h["grad_waypoints"]), q


def test_a_path_gives_the_same_bits_wherever_it_sits(gpu_ctx, groups):
    """the mixed batch reversed, and one path of it alone: rows (headings included), counts, first rows and gradients of every
    path in the same bits"""
    probs = groups["mixed_70"]
    cap = probs[0]["capacity"]
    n, samples, first, so = _forward(gpu_ctx, probs)
    g, _ = _backward(gpu_ctx, probs)
    rev = probs[::-1]
    n_r, samples_r, first_r, so_r = _forward(gpu_ctx, rev)
    g_r, _ = _backward(gpu_ctx, rev)
    P = len(probs)
    for q in range(P):
        r = P - 1 - q
        a, b, ar, br = int(so[q]), int(so[q + 1]), int(so_r[r]), int(so_r[r + 1])
        assert n[q] == n_r[r] and np.array_equal(first[a:b], first_r[ar:br]), q
        k = min(int(n[q]), cap)
        assert fu.same_bits(samples[q, :k], samples_r[r, :k]), q
        assert fu.same_bits(g[a + q:b + q + 1], g_r[ar + r:br + r + 1]), q
    q = 17
    n_1, samples_1, first_1, _ = _forward(gpu_ctx, [probs[q]])
    g_1, _ = _backward(gpu_ctx, [probs[q]])
    a, b = int(so[q]), int(so[q + 1])
    assert n_1[0] == n[q] and np.array_equal(first_1, first[a:b])
    assert fu.same_bits(samples_1[0, :min(int(n[q]), cap)], samples[q, :min(int(n[q]), cap)])
    assert fu.same_bits(g_1, g[a + q:b + q + 1])


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_is_the_harness_in_bits(gpu_ctx, groups, cpu, shape):
    probs = groups[shape]
    g, so = _backward(gpu_ctx, probs)
    for q, h in enumerate(cpu[shape]):
        assert fu.same_bits(g[so[q] + q:so[q + 1] + q + 1], h["grad_waypoints"]), q
    assert np.any(g != 0.0)
    if shape == "mixed_70":   # rows at and beyond min(count, capacity) are never read; a zero upstream gives exact zeros
        cap = probs[0]["capacity"]
        up = fu.pack(probs)[4].copy()
        for q, h in enumerate(cpu[shape]):
            up[q, min(h["count"], cap):] = np.nan
        g_nan, _ = _backward(gpu_ctx, probs, upstream=up)
        assert fu.same_bits(g_nan, g)
        g_zero, _ = _backward(gpu_ctx, probs, upstream=np.zeros_like(up))
        assert fu.same_bits(g_zero, np.zeros_like(g))


CHAIN_SEED = 50


def _chain_margins(chains):
    """on the oracle's own Baca times: the least |t / dt - round(t / dt)| / (t / dt) and the least |t - 0.1| over all segments"""
    lattice, floor = np.inf, np.inf
    for c in chains:
        w = np.array(c["waypoints"])
        w[:, 3] = fu.oracle_unwrap(c["waypoints"])
        lim = np.array(c["limits"], dtype=np.float64)
        lim[[0, 1]] *= c["speed_factor"]
        lim[[3, 4]] *= c["accel_factor"]
        if c["relax"]:
            lim[[2, 5, 8]] = fu.bu.FLT_MAX
        t = fu.po.estimate_times(w, lim, baca=True)
        q = t / c["dt"]
        lattice = min(lattice, float(np.min(np.abs(q - np.round(q)) / q)))
        floor = min(floor, float(np.min(np.abs(t - 0.1))))
    return lattice, floor


@pytest.mark.parametrize("shape", SHAPES)
def test_the_whole_chain_on_the_device_is_the_oracle(gpu_ctx, shape):
    """autograd.fallback_trajectory (unwrap, limits, Baca clock, rows: nothing comes down in between) against
    mto_fallback_sampling: equal counts and bit-equal x, y, z for EVERY path, headings within the bound.  The device's Baca
    times are within 1e-13 of the host's, so the counts agree when no segment sits within 1e-9 of a count's edge: asserted on
    the oracle's own times first."""
    batch = fu.shapes()[shape]
    cap = 4096
    chains = fu.chains(batch, CHAIN_SEED, capacity=cap, uniform=True)
    lattice, floor = _chain_margins(chains)
    assert lattice >= 1e-9 and floor >= 1e-9, (lattice, floor)
    so = np.concatenate([[0], np.cumsum([c["waypoints"].shape[0] - 1 for c in chains])]).astype(np.int32)
    wp = np.concatenate([c["waypoints"] for c in chains])
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp_d = _dev(wp)
        samples, n = autograd.fallback_trajectory(plan, wp_d, _dev(np.stack([c["limits"] for c in chains])), 0.2, cap,
                                                  stop_at=_dev(np.concatenate([c["stop_at"] for c in chains])),
                                                  relax_heading=_dev(np.array([c["relax"] for c in chains])),
                                                  speed_factor=0.75, accel_factor=0.5, stopping_time=2.0)
        out = torch.full_like(wp_d, SENTINEL)
        plan.unwrap_headings(wp_d, out)
        inplace = wp_d.clone()
        plan.unwrap_headings(inplace)
        torch.cuda.synchronize()
    finally:
        plan.close()
    samples, n, out, inplace = samples.cpu().numpy(), n.cpu().numpy(), out.cpu().numpy(), inplace.cpu().numpy()
    worst = 0.0
    for q, c in enumerate(chains):
        count, ref = fu.oracle_chain(c)
        assert count <= cap and int(n[q]) == count, (q, int(n[q]), count)
        assert fu.same_bits(samples[q, :count, :3], ref[:, :3]), q
        assert np.all(samples[q, count:] == 0.0)
        d = fu.wrapped_difference(samples[q, :count, 3], ref[:, 3])
        worst = max(worst, float(d.max()))
        assert np.all(d <= fu.HEADING_BOUND), (q, float(d.max()))
        a, b = int(so[q]) + q, int(so[q + 1]) + q + 1
        want = np.array(c["waypoints"])
        want[:, 3] = fu.oracle_unwrap(c["waypoints"])
        assert fu.same_bits(out[a:b], want) and fu.same_bits(inplace[a:b], want), q
    print("FALLBACK GPU CHAIN %s: worst heading difference %.3e = %.3f of the bound; margins %.2e, %.2e"
          % (shape, worst, worst / fu.HEADING_BOUND, lattice, floor))


def test_autograd_against_central_differences_of_the_gpu_forward(gpu_ctx, groups):
    """L = sum G . samples[..., :3] with |G| = 1 is linear in x, y, z of the waypoints (the times, so the counts, are inputs).
    Along a direction D the difference quotient (L(w + h D) - L(w - h D)) / width is <grad, D> up to the roundings of L: every
    row element a + c (b - a) carries three roundings at a magnitude of at most |a| + |b| <= 2 W (W the largest perturbed
    coordinate), the products with G = +-1 and the sum (math.fsum) are exact, so |L - exact| <= 6 u N W with N elements and
    u = 2^-53, and the difference L(w + h D) - L(w - h D) carries two of them.  It is compared, undivided, with <grad, (w + h D)
    - (w - h D)>, whose own roundings (the gradient's sums, at most u sum|addends| a step, times a width of 2 h |D| <= 2 h) are
    covered by 2 u N h a side.  Bound on the difference: 2 u (6 N W + 2 N h); as a quotient, that over 2 h."""
    probs = groups["mixed_70"]
    so, wp_h, stop, times, _ = fu.pack(probs)
    cap, p0, P = probs[0]["capacity"], probs[0], len(probs)
    rng = np.random.default_rng(77)
    G = np.zeros((P, cap, 4))
    G[:, :, :3] = rng.choice([-1.0, 1.0], size=(P, cap, 3))
    h = 2.0 ** -6
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        t_d, stop_d, G_d = _dev(times), _dev(stop), _dev(G)

        def rows(w):
            s, n = autograd.fallback_sample(plan, _dev(w), t_d, p0["dt"], cap, stop_at=stop_d, stopping_time=p0["stopping_time"])
            torch.cuda.synchronize()
            return s.cpu().numpy(), n.cpu().numpy()

        wp = _dev(wp_h).requires_grad_(True)
        s, n = autograd.fallback_sample(plan, wp, t_d, p0["dt"], cap, stop_at=stop_d, stopping_time=p0["stopping_time"])
        (s * G_d).sum().backward()
        torch.cuda.synchronize()
        grad = wp.grad.cpu().numpy()
        worst = 0.0
        for trial in range(3):
            D = np.zeros_like(wp_h)
            D[:, :3] = rng.uniform(-1.0, 1.0, size=(wp_h.shape[0], 3))
            up, dn = wp_h + h * D, wp_h - h * D
            width = (up - wp_h) + (wp_h - dn)                     # what the two perturbed inputs really are apart
            Dw = np.where(D != 0, width / np.where(D != 0, D, 1.0), 0.0)
            assert np.all(Dw[:, :3] > 0)
            (s_up, n_up), (s_dn, n_dn) = rows(up), rows(dn)
            assert np.array_equal(n_up, n_dn) and np.array_equal(n_up, n.cpu().numpy())
            L_up, L_dn = math.fsum((s_up * G).ravel().tolist()), math.fsum((s_dn * G).ravel().tolist())
            analytic = math.fsum((grad * width).ravel().tolist())     # <grad, up - dn>
            N = 3 * int(np.minimum(n_up, cap).sum())
            W = float(np.abs(np.concatenate([up[:, :3], dn[:, :3]])).max())
            bound = (6 * N * W + 2 * N * h) * 2.0 ** -53 * 2            # both sides of the quotient, not yet divided by 2 h
            worst = max(worst, abs((L_up - L_dn) - analytic) / bound)
            assert abs((L_up - L_dn) - analytic) <= bound, (trial, L_up - L_dn, analytic, bound)
    finally:
        plan.close()
    assert np.abs(grad[:, :3]).max() > 1.0 and np.all(grad[:, 3] == 0.0)
    print("FALLBACK GPU CENTRAL DIFFERENCES: worst |difference| / bound %.3f" % worst)


def test_autograd_is_wired_to_the_backward_call_bit_for_bit(gpu_ctx, groups):
    probs = groups["mixed_70"]
    so, wp_h, stop, times, up = fu.pack(probs)
    cap, p0 = probs[0]["capacity"], probs[0]
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp = _dev(wp_h).requires_grad_(True)
        t = _dev(times).requires_grad_(True)
        s, n = autograd.fallback_sample(plan, wp, t, p0["dt"], cap, stop_at=_dev(stop), stopping_time=p0["stopping_time"])
        (s * _dev(up)).sum().backward()
        direct = torch.empty_like(wp)
        plan.fallback_sample_vjp(_dev(times), p0["dt"], cap, _dev(up), direct, stop_at=_dev(stop),
                                 stopping_time=p0["stopping_time"])
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert t.grad is None                      # the counts are held fixed
    assert fu.same_bits(wp.grad.cpu().numpy(), direct.cpu().numpy()) and bool(torch.any(direct != 0))
    assert n.dtype == torch.int32 and not n.requires_grad


def test_the_chain_into_path_deviation_backpropagates(gpu_ctx, groups):
    probs = groups["uniform_70x3"]
    so, wp_h, stop, times, _ = fu.pack(probs)
    cap, p0 = probs[0]["capacity"], probs[0]
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp = _dev(wp_h).requires_grad_(True)
        s, n = autograd.fallback_sample(plan, wp, _dev(times), p0["dt"], cap, stop_at=_dev(stop),
                                        stopping_time=p0["stopping_time"])
        target = _dev(wp_h + np.array([0.3, -0.2, 0.1, 0.0]))       # the polyline moved aside: the rows stray from it
        dev, _ = autograd.path_deviation(plan, s, n, target)
        dev.sum().backward()
        torch.cuda.synchronize()
    finally:
        plan.close()
    g = wp.grad.cpu().numpy()
    assert g.shape == wp_h.shape and np.all(np.isfinite(g)) and np.any(g[:, :3] != 0.0)
    assert float(dev.detach().sum()) > 0.0


def test_argument_errors_launch_nothing(gpu_ctx, groups):
    probs = groups["uniform_3x1"]
    so, wp_h, stop, times, up = fu.pack(probs)
    cap = probs[0]["capacity"]
    P = len(probs)
    L = api.load_library()
    plan = api.Plan(gpu_ctx, so)
    try:
        gpu_ctx.use_torch_stream()
        wp, t, st, up_d = _dev(wp_h), _dev(times), _dev(stop), _dev(up)
        n = torch.full((P,), ISENTINEL, dtype=torch.int32, device="cuda")
        s = torch.full((P, cap, 4), SENTINEL, dtype=torch.float64, device="cuda")
        g = torch.full((int(so[-1]) + P, 4), SENTINEL, dtype=torch.float64, device="cuda")
        ptr = api._t_ptr

        def fwd(dt=0.2, stopping=2.0, capacity=cap, w=wp, tt=t, nn=n, ss=s):
            return L.mrs_tg_plan_fallback_sample(plan._h, ptr(w), ptr(st), ptr(tt), dt, stopping, capacity, ptr(nn), ptr(ss), None)

        def bwd(dt=0.2, stopping=2.0, capacity=cap, tt=t, uu=up_d, gg=g):
            return L.mrs_tg_plan_fallback_sample_vjp(plan._h, ptr(st), ptr(tt), dt, stopping, capacity, ptr(uu), ptr(gg))

        api.kernel_trace_reset()
        for call in (fwd, bwd):
            for kw in (dict(dt=0.0), dict(dt=-0.2), dict(dt=float("nan")), dict(dt=float("inf")), dict(stopping=-1.0),
                       dict(stopping=float("nan")), dict(stopping=float("inf")), dict(dt=1e-12, stopping=1.0),
                       dict(capacity=0), dict(capacity=-3), dict(capacity=2 ** 31 - 1), dict(tt=None)):
                assert call(**kw) == INVALID_ARG, (call.__name__, kw)
        for kw in (dict(w=None), dict(nn=None), dict(ss=None)):
            assert fwd(**kw) == INVALID_ARG, kw
        for kw in (dict(uu=None), dict(gg=None)):
            assert bwd(**kw) == INVALID_ARG, kw
        assert L.mrs_tg_plan_unwrap_headings(plan._h, None, ptr(wp)) == INVALID_ARG
        assert L.mrs_tg_plan_unwrap_headings(plan._h, ptr(wp), None) == INVALID_ARG
        for kw in (dict(waypoints=wp[:-1]), dict(waypoints=wp[:, :3].contiguous()), dict(stop_at=st[:-1]),
                   dict(relax_heading=torch.zeros(P + 1, dtype=torch.bool, device="cuda"))):     # the wrapper checks shapes first
            args = dict(waypoints=wp, stop_at=st, relax_heading=None)
            args.update(kw)
            with pytest.raises(ValueError):
                autograd.fallback_trajectory(plan, args["waypoints"], _dev(np.ones((P, 9))), 0.2, cap, stop_at=args["stop_at"],
                                             relax_heading=args["relax_heading"])
        assert api.kernel_trace() == []
        torch.cuda.synchronize()
        assert bool(torch.all(n == ISENTINEL)) and bool(torch.all(s == SENTINEL)) and bool(torch.all(g == SENTINEL))
        assert fwd() == 0 and bwd() == 0 and fwd(stopping=0.0) == 0
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["fallback_sample_kernel", "fallback_sample_vjp_kernel", "fallback_sample_kernel"]
    finally:
        plan.close()

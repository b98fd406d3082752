"""mrs_tg_plan_travel_heading / mrs_tg_plan_travel_heading_vjp on the GPU (travel_heading_kernel, travel_heading_vjp_kernel,
DESIGN.md section 11f) and autograd.travel_heading on top of them, on the named cases of tests/heading_util.py: sources against
the numpy restatement of the reference's loop exactly, x, y, z and every row the stage does not own bit for bit, carried headings
as copies of their source's, source headings within the measured bound of np.arctan2, in place against out of place, two calls
against each other, the backward pass against the CPU harness bit for bit and against torch's autograd, and the chain solve ->
sample -> travel_heading -> loss.  A NaN coordinate is ordinary data here: nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import deviation_util as du
from tests import heading_util as hu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
INVALID_ARG = -1


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a) if dtype is None else np.ascontiguousarray(a, dtype=dtype)).cuda()


def _guarded(rows, tail, dtype, fill):
    """a tensor with one guard path in front and one behind, and the view between them that the call gets"""
    full = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device="cuda")
    return full, full[1:rows + 1]


def _guards_untouched(full, fill, name):
    host = full.cpu().numpy()
    assert np.all(host[0] == fill) and np.all(host[-1] == fill), "%s: a neighbour of the plan's rows was written" % name
    return host[1:-1].copy()


def _run_case(ctx, batch):
    """every call the tests look at, once per case"""
    samples, n, status, upstream = hu.batch_arrays(batch)
    P, cap = samples.shape[:2]
    plan = api.Plan(ctx, np.arange(P + 1, dtype=np.int32))
    try:
        ctx.use_torch_stream()
        s_d, n_d, st_d, up_d = _dev(samples), _dev(n), _dev(status), _dev(upstream)
        out = {}
        for call in ("first", "second"):
            o_full, o_view = _guarded(P, (cap, 4), torch.float64, SENTINEL)
            i_full, i_view = _guarded(P, (cap,), torch.int32, ISENTINEL)
            plan.travel_heading(s_d, n_d, samples_out=o_view, status=st_d, source=i_view)
            g_full, g_view = _guarded(P, (cap, 4), torch.float64, SENTINEL)
            plan.travel_heading_vjp(s_d, n_d, up_d, g_view, status=st_d)
            torch.cuda.synchronize()
            out[call] = dict(rows=_guards_untouched(o_full, SENTINEL, "samples_out"),
                             source=_guards_untouched(i_full, ISENTINEL, "source_out"),
                             grad=_guards_untouched(g_full, SENTINEL, "grad_samples"))
        p_full, p_view = _guarded(P, (cap, 4), torch.float64, SENTINEL)
        p_view.copy_(s_d)
        plan.travel_heading(p_view, n_d, status=st_d)                       # in place, no source wanted
        torch.cuda.synchronize()
        out["in_place"] = _guards_untouched(p_full, SENTINEL, "samples (in place)")
        assert np.array_equal(s_d.cpu().numpy().view(np.int64), samples.view(np.int64)), "an input was written"
    finally:
        plan.close()
    out.update(samples=samples, n=n, status=status, upstream=upstream,
               m=[hu.live_rows(n[q], status[q], cap) for q in range(P)])
    return out


@pytest.fixture(scope="module")
def cases():
    return hu.named_cases()


@pytest.fixture(scope="module")
def cpu(cases, tmp_path_factory):
    exe = hu.build_harness(tmp_path_factory.mktemp("heading_gpu"))
    return {name: hu.run_harness(exe, batch) for name, batch in cases.items()}


@pytest.fixture(scope="module")
def gpu(gpu_ctx, cases):
    return {name: _run_case(gpu_ctx, batch) for name, batch in cases.items()}


def _paths(gpu):
    for name, g in gpu.items():
        for q, m in enumerate(g["m"]):
            yield name, q, m, g


def test_capability_bit_is_set():
    assert api.capabilities() & api.CAP_TRAVEL_HEADING and api.CAP_TRAVEL_HEADING == 8192


def test_sources_are_the_reference_loops(gpu):
    rows = 0
    for name, q, m, g in _paths(gpu):
        _, source = hu.travel_heading_numpy(g["samples"][q, :m])
        got = g["first"]["source"][q]
        assert np.array_equal(got[:m], source), (name, q)
        assert np.all(got[m:] == ISENTINEL), (name, q)
        rows += m
    assert rows > 1500


def test_positions_and_the_rows_the_stage_does_not_own_keep_their_bits(gpu):
    for name, q, m, g in _paths(gpu):
        s, o, ip = g["samples"][q], g["first"]["rows"][q], g["in_place"][q]
        assert hu.same_bits(o[:m, :3], s[:m, :3]), (name, q)
        if m:
            assert hu.same_bits(o[m - 1], s[m - 1]), (name, q)                 # the last row keeps its sampled yaw
        assert np.all(o[m:] == SENTINEL), (name, q)                            # rows from n on, and a dead path's, are not written
        assert hu.same_bits(ip[:, :3], s[:, :3]) and hu.same_bits(ip[max(m - 1, 0):], s[max(m - 1, 0):]), (name, q)


def test_a_carried_heading_is_a_copy_of_its_sources(gpu):
    carried = 0
    for name, q, m, g in _paths(gpu):
        h, src = g["first"]["rows"][q, :m, 3], g["first"]["source"][q, :m]
        if m > 1:
            assert hu.same_bits(h[:m - 1], h[src[:m - 1]]), (name, q)
            carried += int(np.sum(src[:m - 1] != np.arange(m - 1)))
    assert carried > 300


def test_source_headings_are_within_the_measured_bound_of_arctan2(gpu):
    worst, count = 0.0, 0
    for name, q, m, g in _paths(gpu):
        want, source = hu.travel_heading_numpy(g["samples"][q, :m])
        got = g["first"]["rows"][q, :m, 3]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, q)
        own = np.flatnonzero((source == np.arange(m)) & ~np.isnan(want))
        if own.size:
            worst = max(worst, float(np.max(np.abs(got[own] - want[own]))))   # directly, not cyclically: the same operands
            count += own.size
    print("TRAVEL HEADING GPU: %d source rows, worst |device atan2 - np.arctan2| %.3e (bound %.3e)" % (count, worst, hu.HEADING_BOUND))
    assert count > 1000 and worst <= hu.HEADING_BOUND
    # signed zeros and the axes come out as the C library's
    h = gpu["negative_zero_dy_is_minus_pi"]["first"]["rows"][0, :4, 3]
    assert np.all(np.abs(np.abs(h) - np.pi) <= hu.HEADING_BOUND) and np.array_equal(np.sign(h), [-1.0, 1.0, -1.0, 1.0])
    z = gpu["zero_step_at_row_0_then_slow"]
    assert not z["first"]["rows"][0, :z["m"][0] - 1, 3].any()
    e = gpu["step_of_exactly_the_threshold"]["first"]
    assert e["source"][0, :5].tolist() == [0, 1, 1, 3, -1] and e["rows"][0, 1, 3] == 0.0 and e["rows"][0, 2, 3] == 0.0


def test_in_place_and_out_of_place_and_two_calls_give_the_same_bits(gpu):
    for name, q, m, g in _paths(gpu):
        a, b = g["first"], g["second"]
        assert hu.same_bits(a["rows"][q], b["rows"][q]) and np.array_equal(a["source"][q], b["source"][q]), (name, q)
        assert hu.same_bits(a["grad"][q], b["grad"][q]), (name, q)
        assert hu.same_bits(g["in_place"][q, :m], a["rows"][q, :m]), (name, q)


def test_backward_is_the_harness_in_the_same_bits_and_torchs_gradient(gpu, cpu):
    for name, q, m, g in _paths(gpu):
        got = g["first"]["grad"][q]
        assert cpu[name][q]["m"] == m
        assert hu.same_bits(got[:m], cpu[name][q]["grad"]), (name, q)
        assert not got[m:].any(), (name, q)                                   # rows from n on and a dead path's rows are zero
        _, source = hu.travel_heading_numpy(g["samples"][q, :m])
        want = hu.travel_heading_torch_grad(g["samples"][q, :m], g["upstream"][q, :m], source)
        assert hu.grads_agree(got[:m], want, hu.grad_scale(g["samples"][q, :m], g["upstream"][q, :m], source)), (name, q)


def test_arguments_are_checked_before_any_launch(gpu_ctx):
    L = api.load_library()
    plan = api.Plan(gpu_ctx, np.arange(3, dtype=np.int32))
    try:
        s = torch.zeros((2, 8, 4), dtype=torch.float64, device="cuda")
        n = torch.full((2,), 8, dtype=torch.int32, device="cuda")
        g = torch.zeros_like(s)
        ptr = api._t_ptr
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert L.mrs_tg_plan_travel_heading(plan._h, ptr(s), ptr(n), 8, None, bad, ptr(s), None) == INVALID_ARG
            assert L.mrs_tg_plan_travel_heading_vjp(plan._h, ptr(s), ptr(n), 8, None, bad, ptr(g), ptr(g)) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading(plan._h, ptr(s), ptr(n), -1, None, 0.05, ptr(s), None) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading(plan._h, None, ptr(n), 8, None, 0.05, ptr(s), None) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading(plan._h, ptr(s), None, 8, None, 0.05, ptr(s), None) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading(plan._h, ptr(s), ptr(n), 8, None, 0.05, None, None) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading_vjp(plan._h, ptr(s), ptr(n), 8, None, 0.05, None, ptr(g)) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading_vjp(plan._h, ptr(s), ptr(n), 8, None, 0.05, ptr(g), None) == INVALID_ARG
        assert L.mrs_tg_plan_travel_heading(None, ptr(s), ptr(n), 8, None, 0.05, ptr(s), None) == INVALID_ARG
        with pytest.raises(ValueError):
            autograd.travel_heading(plan, s[:1], n)
        api.kernel_trace_reset()
        plan.travel_heading(s, n)
        plan.travel_heading_vjp(s, n, g, torch.empty_like(g))
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["travel_heading_kernel", "travel_heading_vjp_kernel"]
    finally:
        plan.close()


def test_chain_solve_sample_travel_heading_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of a loss on the rows the tracker receives, through solve -> sample ->
    autograd.travel_heading: finite, alive, and the bits of the same chain with the stage's backward pass made by hand --
    dL/d(rows) handed to Plan.travel_heading_vjp, its result pushed on through the sampler and the solve."""
    batch = du.chain_batch()
    cap, dt = du.CHAIN_CAPACITY, du.CHAIN_DT
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    try:
        def chain():
            fv = _dev(batch.fixed_values).requires_grad_(True)
            times = _dev(times0).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, mask, fv, times)
            samples, n = autograd.sample(plan, coeffs, times, dt, cap, status)
            return fv, times, samples, n, status

        def loss_of(rows, n):
            valid = (torch.arange(cap, device=rows.device)[None, :] < n[:, None]).to(torch.float64)
            return ((1.0 - torch.cos(rows[..., 3] - 0.3)) * valid).sum() + 0.1 * ((rows[..., :2] ** 2).sum(-1) * valid).sum()

        fv, times, samples, n, status = chain()
        rows, source = autograd.travel_heading(plan, samples, n, status=status)
        assert rows.requires_grad and not source.requires_grad and rows.data_ptr() != samples.data_ptr()
        loss_of(rows, n).backward()
        # by hand
        fv2, times2, samples2, n2, status2 = chain()
        leaf = rows.detach().clone().requires_grad_(True)
        loss_of(leaf, n2).backward()
        gs = torch.empty_like(samples2)
        gpu_ctx.use_torch_stream()
        plan.travel_heading_vjp(samples2.detach(), n2, leaf.grad.contiguous(), gs, status=status2)
        samples2.backward(gs)
        torch.cuda.synchronize()
        assert bool(torch.all(status > 0)) and bool(torch.all(n == cap + 1))
        src = source.cpu().numpy()
        assert np.all(src[:, :cap - 1] >= 0) and np.all(src[:, cap - 1] == -1)
        assert np.any(src[:, :cap - 1] != np.arange(cap - 1)[None, :])        # a rest-to-rest trajectory starts slowly: carried rows
    finally:
        plan.close()
    for a, b in ((fv, fv2), (times, times2)):
        ga, gb = a.grad.cpu().numpy(), b.grad.cpu().numpy()
        assert np.all(np.isfinite(ga)) and np.any(ga != 0.0)
        assert hu.same_bits(ga, gb)

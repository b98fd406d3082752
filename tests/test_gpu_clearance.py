"""mrs_tg_plan_mutual_clearance / mrs_tg_plan_mutual_clearance_vjp on the GPU (mutual_clearance_kernel,
mutual_clearance_vjp_kernel) and autograd.mutual_clearance on top of them, on the named cases of
tests/clearance_util.py: every forward output and dL/dsamples against the CPU harness bit for bit, case by case and all cases in
one batch with a dead path between; every NULL-output combination, two calls and a rotation of the groups against each other;
the argument checks; and the chain solve -> sample -> mutual_clearance -> hinge.  Only well-formed offsets and partner arrays go
to the device; a NaN coordinate is ordinary data here: nothing provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import clearance_util as cu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
INVALID_ARG = -1
OUTPUTS = ("clearance", "partner", "min_clearance", "argmin")


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


class _Device:
    """a case on the device, with the plan that runs it"""

    def __init__(self, ctx, arr):
        self.arr = arr
        self.P, self.cap = arr["samples"].shape[:2]
        self.plan = api.Plan(ctx, np.arange(self.P + 1, dtype=np.int32))
        self.s, self.n, self.st = _dev(arr["samples"]), _dev(arr["n"]), _dev(arr["status"])
        self.fs, self.off, self.up = _dev(arr["first_step"]), _dev(arr["group_offsets"]), _dev(arr["upstream"])
        self.z = arr["z_scale"]

    def forward(self, want=OUTPUTS):
        """the forward with the outputs named in `want` (the others NULL), every output between guards"""
        P, cap = self.P, self.cap
        shapes = dict(clearance=((cap,), torch.float64, SENTINEL), partner=((cap,), torch.int32, ISENTINEL),
                      min_clearance=((), torch.float64, SENTINEL), argmin=((2,), torch.int32, ISENTINEL))
        bufs = {k: _guarded(P, *shapes[k]) for k in want}
        self.plan.mutual_clearance(self.s, self.n, self.off, first_step=self.fs, status=self.st, z_scale=self.z,
                                   **{k: v[1] for k, v in bufs.items()})
        torch.cuda.synchronize()
        return {k: _guards_untouched(v[0], shapes[k][2], k) for k, v in bufs.items()}

    def backward(self, partner):
        g_full, g_view = _guarded(self.P, (self.cap, 4), torch.float64, SENTINEL)
        self.plan.mutual_clearance_vjp(self.s, self.n, self.off, _dev(partner), self.up, g_view, first_step=self.fs,
                                       status=self.st, z_scale=self.z)
        torch.cuda.synchronize()
        return _guards_untouched(g_full, SENTINEL, "grad_samples")

    def close(self):
        assert np.array_equal(self.s.cpu().numpy().view(np.int64), self.arr["samples"].view(np.int64)), "an input was written"
        self.plan.close()


def _run(ctx, arr, calls=1):
    d = _Device(ctx, arr)
    try:
        out = []
        for _ in range(calls):
            o = d.forward()
            o["grad"] = d.backward(o["partner"])
            out.append(o)
    finally:
        d.close()
    return out if calls > 1 else out[0]


def _same(got, want, name):
    assert cu.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["partner"], want["partner"]), name
    assert cu.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert cu.same_bits(got["grad"], want["grad"]), name


@pytest.fixture(scope="module")
def cases():
    return cu.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cu.build_harness(tmp_path_factory.mktemp("clearance_gpu"))


def test_capability_bit_and_both_kernel_ids_report_a_time(gpu_ctx, cases):
    assert api.capabilities() & api.CAP_MUTUAL_CLEARANCE and api.CAP_MUTUAL_CLEARANCE == 65536
    assert (api.KERNEL_MUTUAL_CLEARANCE, api.KERNEL_MUTUAL_CLEARANCE_VJP) == (35, 36)
    d = _Device(gpu_ctx, cu.batch_arrays(cases["random_groups"]))
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        o = d.forward()
        d.backward(o["partner"])
        assert api.kernel_trace() == ["mutual_clearance_kernel", "mutual_clearance_vjp_kernel"]
        assert gpu_ctx.last_kernel_ms(api.KERNEL_MUTUAL_CLEARANCE) > 0.0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_MUTUAL_CLEARANCE_VJP) > 0.0
    finally:
        gpu_ctx.set_profiling(False)
        d.close()


def test_every_named_case_alone_is_the_harness_in_bits(gpu_ctx, cases, harness):
    rows = 0
    for name, c in cases.items():
        arr = cu.batch_arrays(c)
        got = _run(gpu_ctx, arr)
        _same(got, cu.run_harness(harness, arr), name)
        assert np.array_equal(got["partner"] == -1, np.isinf(got["clearance"])), name
        assert not got["grad"][:, :, 3].any(), name
        rows += int((got["partner"] >= 0).sum())
    assert rows > 4000


@pytest.mark.parametrize("z_scale", [1.0, 0.5])
def test_all_cases_in_one_batch_with_a_dead_path_between_are_the_harness_in_bits(gpu_ctx, cases, harness, z_scale):
    arr = cu.batch_arrays(cu.combined_case(cases, z_scale))
    got = _run(gpu_ctx, arr)
    _same(got, cu.run_harness(harness, arr), "all cases, z_scale %g" % z_scale)
    # ... and a path gets the bits it gets alone, wherever its group sits: every case's slice of the batch, run by itself
    at = 0
    for i, (name, c) in enumerate(cases.items()):
        at += 1 if i else 0                      # the dead path in front
        P = len(c["paths"])
        part = slice(at, at + P)
        alone = _run(gpu_ctx, dict(arr, samples=np.ascontiguousarray(arr["samples"][part]), n=arr["n"][part],
                                   status=arr["status"][part], first_step=arr["first_step"][part],
                                   upstream=np.ascontiguousarray(arr["upstream"][part]), group_offsets=cu.group_offsets_of(c)))
        for key in ("clearance", "min_clearance", "grad"):
            assert cu.same_bits(got[key][part], alone[key]), (name, key)
        assert np.array_equal(np.where(got["partner"][part] >= 0, got["partner"][part] - at, -1), alone["partner"]), name
        assert np.array_equal(got["argmin"][part, 0], alone["argmin"][:, 0]), name
        at += P
    assert at == arr["samples"].shape[0]


def test_every_null_output_combination_changes_no_bit_of_the_others(gpu_ctx, cases):
    d = _Device(gpu_ctx, cu.batch_arrays(cases["random_groups"]))
    try:
        full = d.forward()
        for k in range(1, len(OUTPUTS)):
            for want in itertools.combinations(OUTPUTS, k):
                got = d.forward(want)
                for name in want:
                    assert np.array_equal(got[name].view(np.int64 if got[name].dtype == np.float64 else np.int32),
                                          full[name].view(np.int64 if full[name].dtype == np.float64 else np.int32)), (want, name)
    finally:
        d.close()


def test_two_calls_give_the_same_bits(gpu_ctx, cases):
    for name in ("random_groups", "a_row_that_is_partner_to_several_paths", "groups_3_0_1_5"):
        a, b = _run(gpu_ctx, cu.batch_arrays(cases[name]), calls=2)
        _same(a, b, name)


def test_rotating_the_groups_gives_every_path_the_same_bits(gpu_ctx, cases):
    for name in ("random_groups", "groups_3_0_1_5"):
        c = cases[name]
        rot, order = cu.rotated_case(c)
        cap = cu.capacity_of(c)
        a, b = cu.batch_arrays(c), cu.batch_arrays(rot, capacity=cap)
        b["samples"], b["upstream"] = a["samples"][order], a["upstream"][order]      # (the sentinel rows and the upstream too)
        ga, gb = _run(gpu_ctx, a), _run(gpu_ctx, b)
        new_index = np.argsort(order)
        for key in ("clearance", "min_clearance", "grad"):
            assert cu.same_bits(gb[key], ga[key][order]), (name, key)
        pa = ga["partner"][order]
        assert np.array_equal(gb["partner"], np.where(pa >= 0, new_index[np.maximum(pa, 0)], -1)), name
        assert np.array_equal(gb["argmin"][:, 0], ga["argmin"][order, 0]), name


def test_arguments_are_checked_before_any_launch(gpu_ctx):
    L = api.load_library()
    plan = api.Plan(gpu_ctx, np.arange(3, dtype=np.int32))
    try:
        s = torch.zeros((2, 8, 4), dtype=torch.float64, device="cuda")
        n = torch.full((2,), 8, dtype=torch.int32, device="cuda")
        off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
        c = torch.zeros((2, 8), dtype=torch.float64, device="cuda")
        q = torch.zeros((2, 8), dtype=torch.int32, device="cuda")
        g = torch.zeros_like(s)
        ptr = api._t_ptr

        def shifted(t, nbytes):
            return api.C.c_void_p(t.data_ptr() + nbytes)

        def fwd(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, offsets=ptr(off), n_groups=1, z=1.0, clearance=ptr(c), partner=None):
            return L.mrs_tg_plan_mutual_clearance(plan_h, samples, ns, cap, offsets, n_groups, None, None, z, clearance, partner,
                                                  None, None)

        def vjp(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, offsets=ptr(off), n_groups=1, z=1.0, partner=ptr(q), up=ptr(c),
                out=ptr(g)):
            return L.mrs_tg_plan_mutual_clearance_vjp(plan_h, samples, ns, cap, offsets, n_groups, None, None, z, partner, up, out)

        def refused(rc):
            return rc == INVALID_ARG and len(L.mrs_tg_last_error(gpu_ctx._h)) > 0

        api.kernel_trace_reset()
        for call in (fwd, vjp):
            assert call(plan_h=None) == INVALID_ARG and len(L.mrs_tg_last_error(None)) > 0
            for bad in (dict(samples=None), dict(ns=None), dict(offsets=None), dict(n_groups=-1), dict(cap=-1),
                        dict(z=0.0), dict(z=-1.0), dict(z=float("nan")), dict(z=float("inf")),
                        dict(samples=shifted(s, 8)), dict(ns=shifted(n, 2)), dict(offsets=shifted(off, 1))):
                assert refused(call(**bad)), (call.__name__, bad)
        assert refused(fwd(clearance=None)) and b"NULL" in L.mrs_tg_last_error(gpu_ctx._h)
        assert refused(fwd(clearance=shifted(c, 4))) and refused(fwd(partner=shifted(q, 2)))
        assert refused(vjp(partner=None)) and refused(vjp(up=None)) and refused(vjp(out=None)) and refused(vjp(out=shifted(g, 8)))
        assert api.kernel_trace() == []
        # an empty capacity is a success without a launch
        assert fwd(cap=0) == 0 and vjp(cap=0) == 0 and api.kernel_trace() == []
        # the Python layer: host offsets are checked, the shapes too
        for bad in ([0, 1], [1, 2], [0, 2, 1, 2]):
            with pytest.raises(ValueError):
                plan.mutual_clearance(s, n, bad, clearance=c)
        with pytest.raises(ValueError):
            autograd.mutual_clearance(plan, s[:1], n, [0, 2])
        plan.mutual_clearance(s, n, [0, 2], clearance=c, partner=q)
        plan.mutual_clearance_vjp(s, n, off, q, c, g)
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["mutual_clearance_kernel", "mutual_clearance_vjp_kernel"]
        assert bool(torch.all(c == 0.0)) and bool(torch.all(q[0] == 1)) and bool(torch.all(q[1] == 0)) and not bool(g.any())
    finally:
        plan.close()


def test_chain_solve_sample_mutual_clearance_hinge_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of the hinge relu(R - clearance) through solve -> sample -> mutual_clearance on one
    group of four 4-segment paths, against the same chain whose clearance stage is a float64 torch restatement on the kernel's
    partners.

    The bound.  The two chains share the solve and the sampler (same kernels, same bits); they differ in what the clearance
    stage hands back.  That is checked first, entry by entry: a term g dc/drow is at most eight roundings of relative size eps
    on a difference formed by ONE subtraction of the inputs (no cancellation is amplified), in the kernel and in the
    restatement alike, so the two agree to 16 eps |g| per contributing term, summed over the terms of the row -- its own and
    one per row that names it (cu.term_bound).  Every term has length at most |g|, so this is a relative error of rho = 16 eps
    of every row's contribution, and the final gradients are held to rho times the restatement's own gradient norm, per path,
    as tests/test_gpu_deviation.py::test_chain_solve_sample_deviation_hinge_loss does it.  (Measured on an MI355X: dL/dsamples
    differs by at most 2.2e-16 under bounds of up to 1.1e-14; fixed_values.grad by 3.9e-14 .. 5.4e-14 under bounds of 7.8e-14 ..
    1.0e-13 on gradients of norm 22 .. 29; seg_times.grad by 1.9e-15 .. 1.8e-14 under bounds of 1.2e-14 .. 2.6e-14 on norms
    3.5 .. 7.2; 31 rows per path, all inside the hinge, the least clearance 0.77 m.)"""
    batch = cu.chain_batch()
    cap, dt, R = cu.CHAIN_CAPACITY, cu.CHAIN_DT, cu.CHAIN_RADIUS
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P = batch.n_paths
    v0 = so[:-1] + np.arange(P)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask = _dev(batch.fixed_mask)
    try:
        def chain(stage):
            fv = _dev(batch.fixed_values).requires_grad_(True)
            times = _dev(times0).requires_grad_(True)
            coeffs, _, status = autograd.solve(plan, mask, fv, times)
            samples, n = autograd.sample(plan, coeffs, times, dt, cap, status)
            samples.retain_grad()
            loss, extra = stage(samples, n, status)
            return dict(fv=fv, times=times, samples=samples, n=n, status=status, loss=loss, **extra)

        def kernel_stage(samples, n, status):
            c, partner = autograd.mutual_clearance(plan, samples, n, [0, P], status=status)
            c.retain_grad()
            return torch.relu(R - c).sum(), dict(c=c, partner=partner)

        k = chain(kernel_stage)
        assert k["c"].requires_grad and not k["partner"].requires_grad
        partner = k["partner"].cpu().numpy()
        pr_, rr = np.nonzero(partner >= 0)
        pairs = _dev(np.stack([pr_, rr, partner[pr_, rr], rr], axis=1).astype(np.int64))      # (all paths start at step 0)

        def torch_stage(samples, n, status):
            c = cu.torch_clearance(torch, samples, pairs, 1.0)
            return torch.relu(R - c).sum(), dict(c=c)

        r = chain(torch_stage)
        k["loss"].backward()
        r["loss"].backward()
        torch.cuda.synchronize()
        n = k["n"].cpu().numpy()
        assert bool(torch.all(k["status"] > 0))
        ck, cr = k["c"].detach().cpu().numpy(), r["c"].detach().cpu().numpy()
        live = np.arange(cap)[None, :] < np.minimum(n, cap)[:, None]
        has = partner >= 0                       # (one group, one clock: a live row lacks a neighbour only behind the others' ends)
        assert np.all(live[has]) and np.all(np.isinf(ck[~has])) and has.sum() >= live.sum() - cap
        assert np.max(np.abs(ck[pr_, rr] - cr)) <= 1e-13
        active = has & (ck < R)
        print("CLEARANCE GPU CHAIN: rows per path %s, rows inside the hinge per path %s, least clearance %.3f"
              % (np.minimum(n, cap).tolist(), active.sum(axis=1).tolist(), ck[has].min()))
        assert np.all(active.sum(axis=1) >= 10) and ck[has].min() > 0.1           # the loss is alive on every path
        # the stage's own gradient, entry by entry, within the derived bound
        Gs_k, Gs_r = k["samples"].grad.cpu().numpy(), r["samples"].grad.cpu().numpy()
        arr = dict(samples=k["samples"].detach().cpu().numpy(), n=n.astype(np.int32), status=np.ones(P, dtype=np.int32),
                   first_step=np.zeros(P, dtype=np.int32), group_offsets=np.array([0, P], dtype=np.int32),
                   upstream=k["c"].grad.cpu().numpy(), z_scale=1.0)
        bound = cu.term_bound(arr, partner)
        worst = np.max(np.abs(Gs_k[..., :3] - Gs_r[..., :3]) - bound[..., None])
        print("CLEARANCE GPU CHAIN: dL/dsamples max |diff| %.2e, largest bound %.2e, worst (diff - bound) %.2e"
              % (np.max(np.abs(Gs_k - Gs_r)), bound.max(), worst))
        assert np.all(np.abs(Gs_k[..., :3] - Gs_r[..., :3]) <= bound[..., None])
        assert not Gs_k[..., 3].any() and not Gs_k[~live].any() and np.any(Gs_k[active] != 0.0)
    finally:
        plan.close()
    rho = 16.0 * cu.EPS
    gfk, gfr, gtk, gtr = (x.grad.cpu().numpy() for x in (k["fv"], r["fv"], k["times"], r["times"]))
    worst = []
    for p in range(P):
        vs, ss = slice(v0[p], v0[p] + 5), slice(so[p], so[p + 1])
        ef, et = np.abs(gfk[vs] - gfr[vs]).max(), np.abs(gtk[ss] - gtr[ss]).max()
        nf, nt = np.linalg.norm(gfr[vs]), np.linalg.norm(gtr[ss])
        print("CLEARANCE GPU CHAIN path %d: fixed_values.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e); "
              "seg_times.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e)" % (p, ef, rho * nf, nf, et, rho * nt, nt))
        assert nf > 0 and nt > 0 and np.all(np.isfinite(gfk[vs])) and np.all(np.isfinite(gtk[ss]))
        worst.append((ef - rho * nf, et - rho * nt))
    assert all(f <= 0.0 and t <= 0.0 for f, t in worst), worst


TIE_ROWS = (5, 37, 70, 200, 260)      # at capacity 264: lanes 5 and 37 of wavefront 0, wavefronts 1 and 3, wavefront 0's second chunk


def _tie_case(keep):
    """Subject (path 0) and neighbour (path 2) fly 261 rows side by side up the z axis, a dead path of NaN rows between them in
    the same group; the gap along x is the row's clearance itself: 1 on the rows of `keep`, 2 on the other rows of TIE_ROWS,
    2 .. 3.5 in quarters elsewhere -- every coordinate and every distance exactly representable.  Path 3 is a group of its own:
    no neighbour, every row +inf."""
    m = 261
    gap = 2.0 + 0.25 * (np.arange(m) % 7)
    gap[list(TIE_ROWS)] = 2.0
    gap[list(keep)] = 1.0
    subject = np.zeros((m, 4))
    subject[:, 2] = 0.25 * np.arange(m)
    neighbour = subject.copy()
    neighbour[:, 0] = gap
    lone = subject.copy()
    lone[:, 1] = 64.0
    dead = dict(cu.path(np.full((m, 4), np.nan)), status=0)
    return cu.case([cu.path(subject), dead, cu.path(neighbour), cu.path(lone)], groups=[3, 1])


@pytest.mark.parametrize("first", range(len(TIE_ROWS)))
def test_rows_that_tie_for_the_path_minimum_give_the_lowest_row(gpu_ctx, harness, first):
    """the same double on several rows of one path -- in one wavefront, across wavefronts, in a lane's second chunk: the lowest
    tied row is the argmin, as in the harness"""
    keep = TIE_ROWS[first:]
    arr = cu.batch_arrays(_tie_case(keep))
    assert arr["samples"].shape[1] == 264
    got, want = _run(gpu_ctx, arr), cu.run_harness(harness, arr)
    tied = np.flatnonzero(want["clearance"][0] == want["min_clearance"][0])
    assert tied.tolist() == list(keep) and want["min_clearance"][0] == 1.0 and np.all(want["clearance"][0, :261] >= 1.0)
    _same(got, want, "tie kept on rows %s" % (keep,))
    assert cu.same_bits(got["min_clearance"], [1.0, np.inf, 1.0, np.inf])
    assert got["argmin"].tolist() == [[keep[0], 2], [-1, -1], [keep[0], 0], [-1, -1]]

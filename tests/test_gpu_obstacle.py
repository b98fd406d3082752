"""mrs_tg_plan_obstacle_clearance / mrs_tg_plan_obstacle_clearance_vjp on the GPU (obstacle_clearance_kernel,
obstacle_clearance_vjp_kernel) and autograd.obstacle_clearance on top of them, on the named cases of
tests/obstacle_util.py: every forward output and dL/dsamples against the CPU harness bit for bit, case by case and all cases in
one batch with a dead path between; every NULL-output combination, two calls and a rotation of the paths and of the sets against
each other; the argument checks and the edge counts; and the chain solve -> sample -> obstacle_clearance -> hinge.  Only
well-formed offsets, path_set and nearest arrays go to the device; a NaN coordinate is ordinary data here: nothing provokes a
fault."""
import itertools

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import obstacle_util as ou

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
INVALID_ARG = -1
OUTPUTS = ("clearance", "nearest", "min_clearance", "argmin")


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


def _bits(a):
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


class _Device:
    """a case on the device, with the plan that runs it"""

    def __init__(self, ctx, arr):
        self.arr = arr
        self.P, self.cap = arr["samples"].shape[:2]
        self.plan = api.Plan(ctx, np.arange(self.P + 1, dtype=np.int32))
        self.s, self.n, self.st = _dev(arr["samples"]), _dev(arr["n"]), _dev(arr["status"])
        self.ob, self.off, self.up = _dev(arr["obstacles"]), _dev(arr["set_offsets"]), _dev(arr["upstream"])
        self.ps = None if arr["path_set"] is None else _dev(arr["path_set"])
        self.z = arr["z_scale"]

    def forward(self, want=OUTPUTS):
        """the forward with the outputs named in `want` (the others NULL), every output between guards"""
        P, cap = self.P, self.cap
        shapes = dict(clearance=((cap,), torch.float64, SENTINEL), nearest=((cap,), torch.int32, ISENTINEL),
                      min_clearance=((), torch.float64, SENTINEL), argmin=((2,), torch.int32, ISENTINEL))
        bufs = {k: _guarded(P, *shapes[k]) for k in want}
        self.plan.obstacle_clearance(self.s, self.n, self.ob, self.off, path_set=self.ps, status=self.st, z_scale=self.z,
                                     **{k: v[1] for k, v in bufs.items()})
        torch.cuda.synchronize()
        return {k: _guards_untouched(v[0], shapes[k][2], k) for k, v in bufs.items()}

    def backward(self, nearest):
        g_full, g_view = _guarded(self.P, (self.cap, 4), torch.float64, SENTINEL)
        self.plan.obstacle_clearance_vjp(self.s, self.n, self.ob, self.off, _dev(nearest), self.up, g_view, path_set=self.ps,
                                         status=self.st, z_scale=self.z)
        torch.cuda.synchronize()
        return _guards_untouched(g_full, SENTINEL, "grad_samples")

    def close(self):
        for name, t in (("samples", self.s), ("obstacles", self.ob), ("upstream", self.up)):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(np.ascontiguousarray(self.arr[name]))), "%s was written" % name
        for name, t in (("n", self.n), ("status", self.st), ("set_offsets", self.off)):
            assert np.array_equal(t.cpu().numpy(), self.arr[name]), "%s was written" % name
        self.plan.close()


def _run(ctx, arr, calls=1):
    d = _Device(ctx, arr)
    try:
        out = []
        for _ in range(calls):
            o = d.forward()
            o["grad"] = d.backward(o["nearest"])
            out.append(o)
    finally:
        d.close()
    return out if calls > 1 else out[0]


def _same(got, want, name):
    assert ou.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["nearest"], want["nearest"]), name
    assert ou.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert ou.same_bits(got["grad"], want["grad"]), name


@pytest.fixture(scope="module")
def cases():
    return ou.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ou.build_harness(tmp_path_factory.mktemp("obstacle_gpu"))


def test_capability_bit_and_both_kernel_ids_report_a_time(gpu_ctx, cases):
    assert api.capabilities() & api.CAP_OBSTACLE_CLEARANCE and api.CAP_OBSTACLE_CLEARANCE == 131072
    assert (api.KERNEL_OBSTACLE_CLEARANCE, api.KERNEL_OBSTACLE_CLEARANCE_VJP) == (37, 38)
    d = _Device(gpu_ctx, ou.batch_arrays(cases["random_sets"]))
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        o = d.forward()
        d.backward(o["nearest"])
        assert api.kernel_trace() == ["obstacle_clearance_kernel", "obstacle_clearance_vjp_kernel"]
        assert gpu_ctx.last_kernel_ms(api.KERNEL_OBSTACLE_CLEARANCE) > 0.0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_OBSTACLE_CLEARANCE_VJP) > 0.0
    finally:
        gpu_ctx.set_profiling(False)
        d.close()


def test_every_named_case_alone_is_the_harness_in_bits(gpu_ctx, cases, harness):
    rows = 0
    for name, c in cases.items():
        arr = ou.batch_arrays(c)
        got = _run(gpu_ctx, arr)
        _same(got, ou.run_harness(harness, arr), name)
        assert np.array_equal(got["nearest"] == -1, got["clearance"] == np.inf), name
        assert not got["grad"][:, :, 3].any(), name
        rows += int((got["nearest"] >= 0).sum())
    assert rows > 4000


@pytest.mark.parametrize("z_scale", [1.0, 0.5])
def test_all_cases_in_one_batch_with_a_dead_path_between_are_the_harness_in_bits(gpu_ctx, cases, harness, z_scale):
    whole = ou.combined_case(cases, z_scale)
    arr = ou.batch_arrays(whole)
    got = _run(gpu_ctx, arr)
    _same(got, ou.run_harness(harness, arr), "all cases, z_scale %g" % z_scale)
    # ... and a path gets the bits it gets alone, wherever it sits and wherever its set sits: every case's slice of the batch,
    # run by itself against its own obstacles
    at, ob_at = 0, 0
    for i, (name, c) in enumerate(cases.items()):
        at += 1 if i else 0                      # the dead path in front
        P, M = len(c["paths"]), c["obstacles"].shape[0]
        part = slice(at, at + P)
        alone = _run(gpu_ctx, dict(arr, samples=np.ascontiguousarray(arr["samples"][part]), n=arr["n"][part],
                                   status=arr["status"][part], upstream=np.ascontiguousarray(arr["upstream"][part]),
                                   obstacles=c["obstacles"], set_offsets=ou.set_offsets_of(c),
                                   path_set=None if c["path_set"] is None else np.array(c["path_set"], dtype=np.int32)))
        for key in ("clearance", "min_clearance", "grad"):
            assert ou.same_bits(got[key][part], alone[key]), (name, key)
        assert np.array_equal(np.where(got["nearest"][part] >= 0, got["nearest"][part] - ob_at, -1), alone["nearest"]), name
        assert np.array_equal(got["argmin"][part, 0], alone["argmin"][:, 0]), name
        at += P
        ob_at += M
    assert at == arr["samples"].shape[0] and ob_at == arr["obstacles"].shape[0]


def test_every_null_output_combination_changes_no_bit_of_the_others(gpu_ctx, cases):
    d = _Device(gpu_ctx, ou.batch_arrays(cases["random_sets"]))
    try:
        full = d.forward()
        for k in range(1, len(OUTPUTS)):
            for want in itertools.combinations(OUTPUTS, k):
                got = d.forward(want)
                for name in want:
                    assert np.array_equal(_bits(got[name]), _bits(full[name])), (want, name)
    finally:
        d.close()


def test_two_calls_give_the_same_bits(gpu_ctx, cases):
    for name in ("random_sets", "random_one_set_z_scale_0_3", "sets_3_0_1_5", "set_of_257"):
        a, b = _run(gpu_ctx, ou.batch_arrays(cases[name]), calls=2)
        _same(a, b, name)


def test_rotating_the_paths_and_the_sets_gives_every_path_the_same_bits(gpu_ctx, cases):
    for name in ("random_sets", "sets_3_0_1_5"):
        c = cases[name]
        rot, order, new_of_old = ou.rotated_case(c)
        cap = ou.capacity_of(c)
        a, b = ou.batch_arrays(c), ou.batch_arrays(rot, capacity=cap)
        b["samples"], b["upstream"] = a["samples"][order], a["upstream"][order]      # (the sentinel rows and the upstream too)
        assert not np.array_equal(a["obstacles"], b["obstacles"]) and not np.array_equal(a["path_set"], b["path_set"])
        ga, gb = _run(gpu_ctx, a), _run(gpu_ctx, b)
        for key in ("clearance", "min_clearance", "grad"):
            assert ou.same_bits(gb[key], ga[key][order]), (name, key)
        for key in ("nearest", "argmin"):
            old = ga[key][order] if key == "nearest" else ga[key][order, 1]
            new = gb[key] if key == "nearest" else gb[key][:, 1]
            assert np.array_equal(new, np.where(old >= 0, new_of_old[np.maximum(old, 0)], -1)), (name, key)
        assert np.array_equal(gb["argmin"][:, 0], ga["argmin"][order, 0]), name


def test_arguments_are_checked_before_any_launch_and_the_edge_counts(gpu_ctx):
    L = api.load_library()
    plan = api.Plan(gpu_ctx, np.arange(3, dtype=np.int32))
    empty = api.Plan(gpu_ctx, np.zeros(1, dtype=np.int32))
    try:
        s = torch.zeros((2, 8, 4), dtype=torch.float64, device="cuda")
        n = torch.full((2,), 8, dtype=torch.int32, device="cuda")
        ob = torch.tensor([[3.0, 0.0, 0.0, 1.0], [0.0, 4.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")
        off = torch.tensor([0, 2], dtype=torch.int32, device="cuda")
        ps = torch.zeros((2,), dtype=torch.int32, device="cuda")
        c = torch.full((2, 8), SENTINEL, dtype=torch.float64, device="cuda")
        q = torch.full((2, 8), ISENTINEL, dtype=torch.int32, device="cuda")
        mn = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
        am = torch.full((2, 2), ISENTINEL, dtype=torch.int32, device="cuda")
        g = torch.full((2, 8, 4), SENTINEL, dtype=torch.float64, device="cuda")
        ptr = api._t_ptr

        def shifted(t, nbytes):
            return api.C.c_void_p(t.data_ptr() + nbytes)

        def fwd(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, obstacles=ptr(ob), n_ob=2, offsets=ptr(off), n_sets=1,
                path_set=None, status=None, z=1.0, clearance=ptr(c), nearest=None, mini=None, argmin=None):
            return L.mrs_tg_plan_obstacle_clearance(plan_h, samples, ns, cap, obstacles, n_ob, offsets, n_sets, path_set, status, z,
                                                    clearance, nearest, mini, argmin)

        def vjp(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, obstacles=ptr(ob), n_ob=2, offsets=ptr(off), n_sets=1,
                path_set=None, status=None, z=1.0, nearest=ptr(q), up=ptr(c), out=ptr(g)):
            return L.mrs_tg_plan_obstacle_clearance_vjp(plan_h, samples, ns, cap, obstacles, n_ob, offsets, n_sets, path_set, status,
                                                        z, nearest, up, out)

        def refused(rc):
            return rc == INVALID_ARG and len(L.mrs_tg_last_error(gpu_ctx._h)) > 0

        api.kernel_trace_reset()
        for call in (fwd, vjp):
            assert call(plan_h=None) == INVALID_ARG and len(L.mrs_tg_last_error(None)) > 0
            for bad in (dict(samples=None), dict(ns=None), dict(offsets=None), dict(obstacles=None), dict(n_ob=-1),
                        dict(n_sets=-1), dict(cap=-1), dict(z=0.0), dict(z=-1.0), dict(z=float("nan")), dict(z=float("inf")),
                        dict(samples=shifted(s, 8)), dict(obstacles=shifted(ob, 8)), dict(ns=shifted(n, 2)),
                        dict(offsets=shifted(off, 1)), dict(path_set=shifted(ps, 2)), dict(status=shifted(ps, 1))):
                assert refused(call(**bad)), (call.__name__, bad)
        assert refused(fwd(clearance=None)) and b"NULL" in L.mrs_tg_last_error(gpu_ctx._h)
        assert refused(fwd(clearance=shifted(c, 4))) and refused(fwd(nearest=shifted(q, 2)))
        assert refused(fwd(mini=shifted(mn, 4))) and refused(fwd(argmin=shifted(am, 2)))
        assert refused(vjp(nearest=None)) and refused(vjp(up=None)) and refused(vjp(out=None))
        assert refused(vjp(out=shifted(g, 8))) and refused(vjp(up=shifted(c, 4))) and refused(vjp(nearest=shifted(q, 2)))
        assert api.kernel_trace() == []
        # an empty capacity and an empty plan are successes without a launch, and nothing is written
        assert fwd(cap=0) == 0 and vjp(cap=0) == 0 and api.kernel_trace() == []
        assert fwd(plan_h=empty._h, nearest=ptr(q), mini=ptr(mn), argmin=ptr(am)) == 0 and vjp(plan_h=empty._h) == 0
        assert api.kernel_trace() == []
        torch.cuda.synchronize()
        assert bool(torch.all(c == SENTINEL)) and bool(torch.all(q == ISENTINEL)) and bool(torch.all(g == SENTINEL))
        assert bool(torch.all(mn == SENTINEL)) and bool(torch.all(am == ISENTINEL))
        # no obstacles, and no sets: the kernel runs and writes +inf / -1 everywhere
        off0 = torch.zeros(2, dtype=torch.int32, device="cuda")
        up = torch.ones((2, 8), dtype=torch.float64, device="cuda")
        for kw in (dict(n_ob=0, obstacles=None, offsets=ptr(off0)), dict(n_sets=0)):
            c.fill_(SENTINEL), q.fill_(ISENTINEL), mn.fill_(SENTINEL), am.fill_(ISENTINEL), g.fill_(SENTINEL)
            api.kernel_trace_reset()
            assert fwd(nearest=ptr(q), mini=ptr(mn), argmin=ptr(am), **kw) == 0
            assert vjp(up=ptr(up), **kw) == 0
            torch.cuda.synchronize()
            assert api.kernel_trace() == ["obstacle_clearance_kernel", "obstacle_clearance_vjp_kernel"]
            assert bool(torch.all(c == float("inf"))) and bool(torch.all(q == -1)) and bool(torch.all(mn == float("inf")))
            assert bool(torch.all(am == -1)) and not bool(g.any())
        # the Python layer: host offsets are checked, dtypes, devices, contiguity and shapes too
        for bad in ([0, 1], [1, 2], [0, 2, 1, 2]):
            with pytest.raises(ValueError):
                plan.obstacle_clearance(s, n, ob, bad, clearance=c)
        for kw in (dict(samples=s[:1]), dict(samples=s.float()), dict(samples=s.cpu()), dict(samples=s.transpose(0, 1)),
                   dict(n_samples=n.long()), dict(n_samples=n[:1]), dict(obstacles=ob[:, :3]), dict(obstacles=ob.float()),
                   dict(obstacles=ob.cpu()), dict(path_set=ps.long()), dict(path_set=ps[:1]), dict(status=ps.cpu()),
                   dict(clearance=c[:, :7]), dict(clearance=c.float()), dict(nearest=q.long()), dict(min_clearance=mn[:1]),
                   dict(argmin=am[:, :1]), dict(set_offsets=off.long())):
            args = dict(samples=s, n_samples=n, obstacles=ob, set_offsets=off, clearance=c)
            args.update(kw)
            with pytest.raises(ValueError):
                plan.obstacle_clearance(**args)
        for kw in (dict(nearest=q.long()), dict(grad_clearance=c[:1]), dict(grad_samples=g[:, :, :3]), dict(grad_samples=None),
                   dict(nearest=None), dict(obstacles=ob.t())):
            args = dict(samples=s, n_samples=n, obstacles=ob, set_offsets=off, nearest=q, grad_clearance=c, grad_samples=g)
            args.update(kw)
            with pytest.raises(ValueError):
                plan.obstacle_clearance_vjp(**args)
        with pytest.raises(ValueError):
            autograd.obstacle_clearance(plan, s[:1], n, ob)
        with pytest.raises(ValueError):
            autograd.obstacle_clearance(plan, s, n, ob[:, :3])
        api.kernel_trace_reset()
        plan.obstacle_clearance(s, n, ob, [0, 2], clearance=c, nearest=q)
        c_up = torch.ones_like(c)
        plan.obstacle_clearance_vjp(s, n, ob, off, q, c_up, g, path_set=ps)
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["obstacle_clearance_kernel", "obstacle_clearance_vjp_kernel"]
        # rows at the origin: the sphere of 1 m at 3 m is 2 m away, the point at 4 m is not nearer
        assert bool(torch.all(c == 2.0)) and bool(torch.all(q == 0))
        assert bool(torch.all(g[..., 0] == -1.0)) and not bool(g[..., 1:].any())
    finally:
        plan.close()
        empty.close()


def test_asking_for_a_gradient_of_the_obstacles_raises(gpu_ctx):
    plan = api.Plan(gpu_ctx, np.arange(2, dtype=np.int32))
    try:
        s = torch.zeros((1, 4, 4), dtype=torch.float64, device="cuda", requires_grad=True)
        n = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        ob = torch.tensor([[3.0, 0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda", requires_grad=True)
        with pytest.raises(ValueError, match="static map"):
            autograd.obstacle_clearance(plan, s, n, ob)
        c, nearest = autograd.obstacle_clearance(plan, s, n, ob.detach())          # set_offsets None: one set, the whole map
        assert c.requires_grad and not nearest.requires_grad
        c.sum().backward()
        torch.cuda.synchronize()
        assert bool(torch.all(c == 2.0)) and bool(torch.all(nearest == 0))
        assert bool(torch.all(s.grad[..., 0] == -1.0)) and not bool(s.grad[..., 1:].any()) and ob.grad is None
    finally:
        plan.close()


def test_chain_solve_sample_obstacle_clearance_hinge_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of the hinge relu(R - clearance) through solve -> sample -> obstacle_clearance on
    three 4-segment paths and nine obstacles, against the same chain with the torch composition in place of the step: the
    [N][Q][M] broadcast of sqrt(...) - radius, torch.min over the obstacles, a mask over the live rows.

    The bound.  The two chains share the solve and the sampler (same kernels, same bits); they differ in what the clearance
    stage hands back.  That is checked first, entry by entry: an entry of dL/dsamples is ONE term g d_k / s, so the sum of its
    absolute terms is the term's own size, and the two are held to 1e-13 of it (ou.GRAD_RTOL, the bound
    tests/test_obstacle_host.py holds the harness to torch with: a few roundings of relative size 2^-53 on a difference formed
    by one subtraction of the inputs on both sides).  This is a relative error rho = 1e-13 of every row's contribution, and
    the final gradients are held to rho times the composition's own gradient norm, per path, as
    tests/test_gpu_clearance.py::test_chain_solve_sample_mutual_clearance_hinge_loss does it.  The figures are printed."""
    batch, obstacles = ou.chain_batch()
    cap, dt, R = ou.CHAIN_CAPACITY, ou.CHAIN_DT, ou.CHAIN_RADIUS
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P = batch.n_paths
    assert P == 3 and np.all(np.diff(so) == 4) and obstacles.shape == (9, 4)
    v0 = so[:-1] + np.arange(P)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask, ob = _dev(batch.fixed_mask), _dev(obstacles)
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
            c, nearest = autograd.obstacle_clearance(plan, samples, n, ob, status=status)
            c.retain_grad()
            return torch.relu(R - c).sum(), dict(c=c, nearest=nearest)        # (no mask: +inf behind a path's last row)

        def torch_stage(samples, n, status):
            d = samples[:, :, None, :3] - ob[None, None, :, :3]
            c_all = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2) - ob[None, None, :, 3]
            c, nearest = c_all.min(dim=2)
            valid = torch.arange(cap, device=samples.device)[None, :] < torch.clamp(n, max=cap)[:, None]
            c.retain_grad()
            return (torch.relu(R - c) * valid).sum(), dict(c=c, nearest=nearest)

        k, r = chain(kernel_stage), chain(torch_stage)
        assert k["c"].requires_grad and not k["nearest"].requires_grad
        k["loss"].backward()
        r["loss"].backward()
        torch.cuda.synchronize()
        n = k["n"].cpu().numpy()
        assert bool(torch.all(k["status"] > 0))
        ck, cr = k["c"].detach().cpu().numpy(), r["c"].detach().cpu().numpy()
        nk, nr = k["nearest"].cpu().numpy(), r["nearest"].cpu().numpy()
        live = np.arange(cap)[None, :] < np.minimum(n, cap)[:, None]
        assert np.all(nk[live] >= 0) and np.all(nk[~live] == -1) and np.all(ck[~live] == np.inf)
        assert np.array_equal(nk[live], nr[live]) and np.max(np.abs(ck[live] - cr[live])) <= 1e-13
        active = live & (ck < R)
        print("OBSTACLE GPU CHAIN: rows per path %s, rows inside the hinge per path %s, least clearance %.3f, obstacles that are "
              "somebody's nearest %d" % (np.minimum(n, cap).tolist(), active.sum(axis=1).tolist(), ck[live].min(),
                                         len(np.unique(nk[live]))))
        assert np.all(active.sum(axis=1) >= 10) and ck[live].min() > 0.1           # the loss is alive on every path
        # the stage's own gradient, entry by entry, within 1e-13 of the sum of its absolute terms
        Gs_k, Gs_r = k["samples"].grad.cpu().numpy(), r["samples"].grad.cpu().numpy()
        arr = dict(samples=k["samples"].detach().cpu().numpy(), n=n.astype(np.int32), status=np.ones(P, dtype=np.int32),
                   obstacles=obstacles, set_offsets=np.array([0, 9], dtype=np.int32), path_set=None,
                   upstream=k["c"].grad.cpu().numpy(), z_scale=1.0)
        _, scale = ou.obstacle_clearance_torch_grad(arr, nk)
        diff = np.abs(Gs_k - Gs_r)
        print("OBSTACLE GPU CHAIN: dL/dsamples max |diff| %.2e, largest bound %.2e, worst (diff - bound) %.2e"
              % (diff.max(), ou.GRAD_RTOL * scale.max(), np.max(diff - ou.GRAD_RTOL * scale)))
        assert ou.grads_agree(Gs_k, Gs_r, scale)
        assert not Gs_k[..., 3].any() and not Gs_k[~live].any() and np.any(Gs_k[active] != 0.0)
    finally:
        plan.close()
    rho = ou.GRAD_RTOL
    gfk, gfr, gtk, gtr = (x.grad.cpu().numpy() for x in (k["fv"], r["fv"], k["times"], r["times"]))
    worst = []
    for p in range(P):
        vs, ss = slice(v0[p], v0[p] + 5), slice(so[p], so[p + 1])
        ef, et = np.abs(gfk[vs] - gfr[vs]).max(), np.abs(gtk[ss] - gtr[ss]).max()
        nf, nt = np.linalg.norm(gfr[vs]), np.linalg.norm(gtr[ss])
        print("OBSTACLE GPU CHAIN path %d: fixed_values.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e); "
              "seg_times.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e)" % (p, ef, rho * nf, nf, et, rho * nt, nt))
        assert nf > 0 and nt > 0 and np.all(np.isfinite(gfk[vs])) and np.all(np.isfinite(gtk[ss]))
        worst.append((ef - rho * nf, et - rho * nt))
    assert all(f <= 0.0 and t <= 0.0 for f, t in worst), worst


TIE_ROWS = (5, 37, 70, 200, 260)      # at capacity 264: lanes 5 and 37 of wavefront 0, wavefronts 1 and 3, lane 4's second row


def _tie_case(keep):
    """One point obstacle at (1, 2, 3) and a path of 261 rows around it: the rows of `keep` on the sphere of radius 4 about it
    (on five different half-axes), the other rows of TIE_ROWS at 8, the rest at 8 .. 9.5 in quarters along x -- every coordinate
    and every distance exactly representable.  Path 1 is dead (NaN rows, the same set); path 2 sees the empty set: every row
    +inf."""
    m = 261
    centre = np.array([1.0, 2.0, 3.0])
    rows = np.zeros((m, 4))
    rows[:, :3] = centre
    rows[:, 0] += 8.0 + 0.25 * (np.arange(m) % 7)
    axes = ([4.0, 0.0, 0.0], [-4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, -4.0, 0.0], [0.0, 0.0, 4.0])
    for r, axis in zip(TIE_ROWS, axes):
        rows[r, :3] = centre + (np.array(axis) if r in keep else [8.0, 0.0, 0.0])
    dead = dict(ou.path(np.full((m, 4), np.nan)), status=0)
    return ou.case([ou.path(rows), dead, ou.path(rows)], [list(centre) + [0.0]], sets=[1, 0], path_set=[0, 0, 1])


@pytest.mark.parametrize("first", range(len(TIE_ROWS)))
def test_rows_that_tie_for_the_path_minimum_give_the_lowest_row(gpu_ctx, harness, first):
    """the same double on several rows of one path -- in one wavefront, across wavefronts, in a lane's second row: the lowest
    tied row is the argmin, as in the harness"""
    keep = TIE_ROWS[first:]
    arr = ou.batch_arrays(_tie_case(keep))
    assert arr["samples"].shape[1] == 264
    got, want = _run(gpu_ctx, arr), ou.run_harness(harness, arr)
    tied = np.flatnonzero(want["clearance"][0] == want["min_clearance"][0])
    assert tied.tolist() == list(keep) and want["min_clearance"][0] == 4.0 and np.all(want["clearance"][0, :261] >= 4.0)
    _same(got, want, "tie kept on rows %s" % (keep,))
    assert ou.same_bits(got["min_clearance"], [4.0, np.inf, np.inf])
    assert got["argmin"].tolist() == [[keep[0], 0], [-1, -1], [-1, -1]]

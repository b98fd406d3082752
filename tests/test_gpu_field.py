"""mrs_tg_plan_field_clearance / mrs_tg_plan_field_clearance_vjp on the GPU (field_clearance_kernel, field_clearance_vjp_kernel,
DESIGN.md section 11k) and autograd.field_clearance on top of them, on the named cases of tests/field_util.py: every forward
output and dL/dsamples against the CPU harness bit for bit, case by case and all cases of one geometry in one batch with a dead
path between; every NULL-output combination, two calls and a rotation of the paths and of the grids against each other; the
argument checks and the edge counts; the field of nine spheres built on the device by Plan.obstacle_clearance over the nodes
and looked up again; and the chain solve -> sample -> field_clearance -> hinge.  Only well-formed path_field and cell arrays go
to the device; a NaN coordinate or voxel is ordinary data here: nothing provokes a fault."""
import itertools

import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import field_util as fu

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = -777.25, -7
INVALID_ARG = -1
OUTPUTS = ("clearance", "cell", "gradient", "min_clearance", "argmin")


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
        self.f, self.up = _dev(arr["fields"]), _dev(arr["upstream"])
        self.g = fu.arrays_geometry(arr)
        self.pf = None if arr["path_field"] is None else _dev(arr["path_field"])
        self.outside = arr["outside_value"]

    def forward(self, want=OUTPUTS):
        """the forward with the outputs named in `want` (the others NULL), every output between guards"""
        P, cap = self.P, self.cap
        shapes = dict(clearance=((cap,), torch.float64, SENTINEL), cell=((cap,), torch.int32, ISENTINEL),
                      gradient=((cap, 4), torch.float64, SENTINEL), min_clearance=((), torch.float64, SENTINEL),
                      argmin=((2,), torch.int32, ISENTINEL))
        bufs = {k: _guarded(P, *shapes[k]) for k in want}
        self.plan.field_clearance(self.s, self.n, self.f, self.g, path_field=self.pf, status=self.st, outside_value=self.outside,
                                  **{k: v[1] for k, v in bufs.items()})
        torch.cuda.synchronize()
        return {k: _guards_untouched(v[0], shapes[k][2], k) for k, v in bufs.items()}

    def backward(self, cell):
        g_full, g_view = _guarded(self.P, (self.cap, 4), torch.float64, SENTINEL)
        self.plan.field_clearance_vjp(self.s, self.n, self.f, self.g, _dev(cell), self.up, g_view, path_field=self.pf,
                                      status=self.st)
        torch.cuda.synchronize()
        return _guards_untouched(g_full, SENTINEL, "grad_samples")

    def close(self):
        for name, t in (("samples", self.s), ("fields", self.f), ("upstream", self.up)):
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(np.ascontiguousarray(self.arr[name]))), "%s was written" % name
        for name, t in (("n", self.n), ("status", self.st)):
            assert np.array_equal(t.cpu().numpy(), self.arr[name]), "%s was written" % name
        self.plan.close()


def _run(ctx, arr, calls=1):
    d = _Device(ctx, arr)
    try:
        out = []
        for _ in range(calls):
            o = d.forward()
            o["grad"] = d.backward(o["cell"])
            out.append(o)
    finally:
        d.close()
    return out if calls > 1 else out[0]


def _same(got, want, name):
    assert fu.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["cell"], want["cell"]), name
    assert fu.same_bits(got["gradient"], want["gradient"]), name
    assert fu.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert fu.same_bits(got["grad"], want["grad"]), name


@pytest.fixture(scope="module")
def cases():
    return fu.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fu.build_harness(tmp_path_factory.mktemp("field_gpu"))


def test_capability_bit_and_both_kernel_ids_report_a_time(gpu_ctx, cases):
    assert api.capabilities() & api.CAP_FIELD_CLEARANCE and api.CAP_FIELD_CLEARANCE == 262144
    assert (api.KERNEL_FIELD_CLEARANCE, api.KERNEL_FIELD_CLEARANCE_VJP) == (39, 40)
    d = _Device(gpu_ctx, fu.batch_arrays(cases["random_fields"]))
    try:
        gpu_ctx.set_profiling(True)
        api.kernel_trace_reset()
        o = d.forward()
        d.backward(o["cell"])
        assert api.kernel_trace() == ["field_clearance_kernel", "field_clearance_vjp_kernel"]
        assert gpu_ctx.last_kernel_ms(api.KERNEL_FIELD_CLEARANCE) > 0.0
        assert gpu_ctx.last_kernel_ms(api.KERNEL_FIELD_CLEARANCE_VJP) > 0.0
    finally:
        gpu_ctx.set_profiling(False)
        d.close()


def test_every_named_case_alone_is_the_harness_in_bits(gpu_ctx, cases, harness):
    rows = 0
    for name, c in cases.items():
        arr = fu.batch_arrays(c)
        got = _run(gpu_ctx, arr)
        _same(got, fu.run_harness(harness, arr), name)
        assert not got["grad"][:, :, 3].any() and not got["gradient"][:, :, 3].any(), name
        assert not got["grad"][got["cell"] == -1].any() and not got["gradient"][got["cell"] == -1].any(), name
        # g * gradient_out and the backward pass: the same bits
        has = got["cell"] >= 0
        with np.errstate(invalid="ignore", over="ignore"):
            product = np.where(arr["upstream"][..., None] == 0.0, 0.0, arr["upstream"][..., None] * got["gradient"][..., :3])
        assert fu.same_bits(got["grad"][..., :3][has], product[has]), name
        rows += int(has.sum())
    assert rows > 3000


@pytest.mark.parametrize("like, outside", [("fields_4", np.inf), ("fields_4", -1.0), ("rows_65", np.nan)])
def test_all_cases_in_one_batch_with_a_dead_path_between_are_the_harness_in_bits(gpu_ctx, cases, harness, like, outside):
    whole, where = fu.combined_case(cases, like, outside)
    assert len(where) >= 5
    arr = fu.batch_arrays(whole)
    got = _run(gpu_ctx, arr)
    _same(got, fu.run_harness(harness, arr), "all cases on the geometry of %s" % like)
    # ... and a path gets the bits it gets alone, wherever it sits and wherever its grid sits: every case's slice of the batch,
    # run by itself against its own grids
    per_grid = int(np.prod(whole["fields"].shape[1:]))
    for name, at, grid_at in where:
        c = cases[name]
        P = len(c["paths"])
        part = slice(at, at + P)
        alone = _run(gpu_ctx, dict(arr, samples=np.ascontiguousarray(arr["samples"][part]), n=arr["n"][part],
                                   status=arr["status"][part], upstream=np.ascontiguousarray(arr["upstream"][part]),
                                   fields=c["fields"],
                                   path_field=None if c["path_field"] is None else np.array(c["path_field"], dtype=np.int32)))
        for key in ("clearance", "gradient", "min_clearance", "grad"):
            assert fu.same_bits(got[key][part], alone[key]), (name, key)
        assert np.array_equal(np.where(got["cell"][part] >= 0, got["cell"][part] - grid_at * per_grid, -1), alone["cell"]), name
        assert np.array_equal(got["argmin"][part, 0], alone["argmin"][:, 0]), name
        assert np.array_equal(np.where(got["argmin"][part, 1] >= 0, got["argmin"][part, 1] - grid_at * per_grid, -1),
                              alone["argmin"][:, 1]), name


def test_every_null_output_combination_changes_no_bit_of_the_others(gpu_ctx, cases):
    d = _Device(gpu_ctx, fu.batch_arrays(cases["random_fields"]))
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
    for name in ("random_fields", "rows_257", "fields_4", "one_nan_voxel"):
        a, b = _run(gpu_ctx, fu.batch_arrays(cases[name]), calls=2)
        _same(a, b, name)


def test_rotating_the_paths_and_the_grids_gives_every_path_the_same_bits(gpu_ctx, cases):
    for name in ("random_fields", "fields_4"):
        c = cases[name]
        rot, order, per_grid = fu.rotated_case(c)
        F = c["fields"].shape[0]
        cap = fu.capacity_of(c)
        a, b = fu.batch_arrays(c), fu.batch_arrays(rot, capacity=cap)
        b["samples"], b["upstream"] = a["samples"][order], a["upstream"][order]      # (the sentinel rows and the upstream too)
        assert not np.array_equal(a["fields"], b["fields"]) and not np.array_equal(a["path_field"], b["path_field"])
        ga, gb = _run(gpu_ctx, a), _run(gpu_ctx, b)
        for key in ("clearance", "gradient", "min_clearance", "grad"):
            assert fu.same_bits(gb[key], ga[key][order]), (name, key)

        def moved(cell):     # a cell of the old array in the new: its grid one down, the first behind the last
            cell = cell.astype(np.int64)
            return np.where(cell >= 0, ((cell // per_grid - 1) % F) * per_grid + cell % per_grid, -1)

        assert np.array_equal(gb["cell"], moved(ga["cell"][order])), name
        assert np.array_equal(gb["argmin"][:, 1], moved(ga["argmin"][order, 1])), name
        assert np.array_equal(gb["argmin"][:, 0], ga["argmin"][order, 0]), name


def test_arguments_are_checked_before_any_launch_and_the_edge_counts(gpu_ctx):
    L = api.load_library()
    plan = api.Plan(gpu_ctx, np.arange(3, dtype=np.int32))
    empty = api.Plan(gpu_ctx, np.zeros(1, dtype=np.int32))
    try:
        s = torch.zeros((2, 8, 4), dtype=torch.float64, device="cuda")
        n = torch.full((2,), 8, dtype=torch.int32, device="cuda")
        # a (2, 3, 4) grid at the origin with unit spacing that holds x + 2 y + 4 z: the rows at (0.5, 0.5, 0.5) read 3.5
        geometry = api.FieldGeometry((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 3, 4), 1)
        nodes = fu.node_coordinates(geometry)
        fl = _dev((nodes[..., 0] + 2.0 * nodes[..., 1] + 4.0 * nodes[..., 2])[None])
        s[..., :3] = 0.5
        ps = torch.zeros((2,), dtype=torch.int32, device="cuda")
        c = torch.full((2, 8), SENTINEL, dtype=torch.float64, device="cuda")
        q = torch.full((2, 8), ISENTINEL, dtype=torch.int32, device="cuda")
        gr = torch.full((2, 8, 4), SENTINEL, dtype=torch.float64, device="cuda")
        mn = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
        am = torch.full((2, 2), ISENTINEL, dtype=torch.int32, device="cuda")
        g = torch.full((2, 8, 4), SENTINEL, dtype=torch.float64, device="cuda")
        ptr = api._t_ptr
        inf, nan = float("inf"), float("nan")

        def shifted(t, nbytes):
            return api.C.c_void_p(t.data_ptr() + nbytes)

        def geo(**kw):
            a = dict(origin=geometry.origin, spacing=geometry.spacing, dims=geometry.dims, n_fields=1)
            a.update(kw)
            return api.C.byref(api.FieldGeometry(**a).as_struct())

        def fwd(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, fields=ptr(fl), geometry=geo(), path_field=None, status=None,
                outside=inf, clearance=ptr(c), cell=None, gradient=None, mini=None, argmin=None):
            return L.mrs_tg_plan_field_clearance(plan_h, samples, ns, cap, fields, geometry, path_field, status, outside, clearance,
                                                 cell, gradient, mini, argmin)

        def vjp(plan_h=plan._h, samples=ptr(s), ns=ptr(n), cap=8, fields=ptr(fl), geometry=geo(), path_field=None, status=None,
                cell=ptr(q), up=ptr(c), out=ptr(g)):
            return L.mrs_tg_plan_field_clearance_vjp(plan_h, samples, ns, cap, fields, geometry, path_field, status, cell, up, out)

        def refused(rc):
            return rc == INVALID_ARG and len(L.mrs_tg_last_error(gpu_ctx._h)) > 0

        api.kernel_trace_reset()
        for call in (fwd, vjp):
            assert call(plan_h=None) == INVALID_ARG and len(L.mrs_tg_last_error(None)) > 0
            for bad in (dict(samples=None), dict(ns=None), dict(geometry=None), dict(fields=None), dict(cap=-1),
                        dict(geometry=geo(n_fields=-1)), dict(geometry=geo(dims=(1, 3, 4))), dict(geometry=geo(dims=(2, 0, 4))),
                        dict(geometry=geo(dims=(2, 3, -5))), dict(geometry=geo(spacing=(0.0, 1.0, 1.0))),
                        dict(geometry=geo(spacing=(1.0, -1.0, 1.0))), dict(geometry=geo(spacing=(1.0, 1.0, nan))),
                        dict(geometry=geo(spacing=(inf, 1.0, 1.0))), dict(geometry=geo(origin=(nan, 0.0, 0.0))),
                        dict(geometry=geo(origin=(0.0, 0.0, -inf))),
                        # more voxels than an int32 cell can name, with the small real buffer, which must not be read
                        dict(geometry=geo(dims=(2048, 1024, 1024))), dict(geometry=geo(dims=(2, 3, 4), n_fields=2 ** 27)),
                        dict(geometry=geo(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), n_fields=2 ** 31 - 1)),
                        dict(samples=shifted(s, 8)), dict(fields=shifted(fl, 4)), dict(ns=shifted(n, 2)),
                        dict(path_field=shifted(ps, 2)), dict(status=shifted(ps, 1))):
                assert refused(call(**bad)), (call.__name__, bad)
        assert refused(fwd(clearance=None)) and b"NULL" in L.mrs_tg_last_error(gpu_ctx._h)
        assert refused(fwd(clearance=shifted(c, 4))) and refused(fwd(cell=shifted(q, 2)))
        assert refused(fwd(gradient=shifted(gr, 8))) and refused(fwd(mini=shifted(mn, 4))) and refused(fwd(argmin=shifted(am, 2)))
        assert refused(vjp(cell=None)) and refused(vjp(up=None)) and refused(vjp(out=None))
        assert refused(vjp(out=shifted(g, 8))) and refused(vjp(up=shifted(c, 4))) and refused(vjp(cell=shifted(q, 2)))
        # the backward's output may not overlap an input
        assert refused(vjp(out=ptr(s))) and b"overlaps" in L.mrs_tg_last_error(gpu_ctx._h)
        assert refused(vjp(up=shifted(g, 64)))
        assert api.kernel_trace() == []
        # an empty capacity and an empty plan are successes without a launch, and nothing is written
        assert fwd(cap=0) == 0 and vjp(cap=0) == 0 and api.kernel_trace() == []
        assert fwd(plan_h=empty._h, cell=ptr(q), gradient=ptr(gr), mini=ptr(mn), argmin=ptr(am)) == 0 and vjp(plan_h=empty._h) == 0
        assert api.kernel_trace() == []
        torch.cuda.synchronize()
        assert bool(torch.all(c == SENTINEL)) and bool(torch.all(q == ISENTINEL)) and bool(torch.all(g == SENTINEL))
        assert bool(torch.all(mn == SENTINEL)) and bool(torch.all(am == ISENTINEL)) and bool(torch.all(gr == SENTINEL))
        # no grids: the kernel runs and writes +inf / -1 everywhere, zeros for the gradients
        up = torch.ones((2, 8), dtype=torch.float64, device="cuda")
        api.kernel_trace_reset()
        assert fwd(cell=ptr(q), gradient=ptr(gr), mini=ptr(mn), argmin=ptr(am), geometry=geo(n_fields=0), fields=None) == 0
        assert vjp(up=ptr(up), geometry=geo(n_fields=0), fields=None) == 0
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["field_clearance_kernel", "field_clearance_vjp_kernel"]
        assert bool(torch.all(c == inf)) and bool(torch.all(q == -1)) and bool(torch.all(mn == inf))
        assert bool(torch.all(am == -1)) and not bool(g.any()) and not bool(gr.any())
        # the Python layer: the geometry is checked against the fields, dtypes, devices, contiguity and shapes too
        for bad in (api.FieldGeometry((0, 0, 0), (1, 1, 1), (4, 3, 2)), api.FieldGeometry((0, 0, 0), (1, 1, 1), (2, 3, 4), 2),
                    api.FieldGeometry((0, 0, 0), (1, 0, 1), (2, 3, 4)), api.FieldGeometry((nan, 0, 0), (1, 1, 1), (2, 3, 4)),
                    ((0, 0, 0), (1, 1, 1), (2, 3, 4), 1), None):
            with pytest.raises(ValueError):
                plan.field_clearance(s, n, fl, bad, clearance=c)
        for kw in (dict(samples=s[:1]), dict(samples=s.float()), dict(samples=s.cpu()), dict(samples=s.transpose(0, 1)),
                   dict(n_samples=n.long()), dict(n_samples=n[:1]), dict(fields=fl[0]), dict(fields=fl.float()),
                   dict(fields=fl.cpu()), dict(fields=fl.transpose(2, 3)), dict(path_field=ps.long()), dict(path_field=ps[:1]),
                   dict(status=ps.cpu()), dict(clearance=c[:, :7]), dict(clearance=c.float()), dict(cell=q.long()),
                   dict(gradient=gr[:, :, :3]), dict(min_clearance=mn[:1]), dict(argmin=am[:, :1])):
            args = dict(samples=s, n_samples=n, fields=fl, geometry=geometry, clearance=c)
            args.update(kw)
            with pytest.raises(ValueError):
                plan.field_clearance(**args)
        for kw in (dict(cell=q.long()), dict(grad_clearance=c[:1]), dict(grad_samples=g[:, :, :3]), dict(grad_samples=None),
                   dict(cell=None), dict(fields=fl[0])):
            args = dict(samples=s, n_samples=n, fields=fl, geometry=geometry, cell=q, grad_clearance=c, grad_samples=g)
            args.update(kw)
            with pytest.raises(ValueError):
                plan.field_clearance_vjp(**args)
        with pytest.raises(ValueError):
            autograd.field_clearance(plan, s[:1], n, fl, geometry)
        with pytest.raises(ValueError):
            autograd.field_clearance(plan, s, n, fl[0], geometry)
        api.kernel_trace_reset()
        plan.field_clearance(s, n, fl, geometry, clearance=c, cell=q, gradient=gr)
        c_up = torch.ones_like(c)
        plan.field_clearance_vjp(s, n, fl, geometry, q, c_up, g, path_field=ps)
        torch.cuda.synchronize()
        assert api.kernel_trace() == ["field_clearance_kernel", "field_clearance_vjp_kernel"]
        assert bool(torch.all(c == 3.5)) and bool(torch.all(q == 0))
        want = torch.tensor([1.0, 2.0, 4.0, 0.0], dtype=torch.float64, device="cuda")
        assert bool(torch.all(g == want)) and bool(torch.all(gr == want))
    finally:
        plan.close()
        empty.close()


def test_asking_for_a_gradient_of_the_field_raises_and_the_minimum_routes_to_its_row(gpu_ctx):
    plan = api.Plan(gpu_ctx, np.arange(2, dtype=np.int32))
    try:
        geometry = api.FieldGeometry((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 3, 4), 1)
        nodes = fu.node_coordinates(geometry)
        field = _dev((nodes[..., 0] + 2.0 * nodes[..., 1] + 4.0 * nodes[..., 2])[None])
        rows = torch.zeros((1, 4, 4), dtype=torch.float64, device="cuda")
        rows[0, :, :3] = torch.tensor([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0.5, 1.5, 2.5], [9.0, 0.5, 0.5]])
        s = rows.clone().requires_grad_(True)
        n = torch.full((1,), 4, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="static map"):
            autograd.field_clearance(plan, s, n, field.clone().requires_grad_(True), geometry)
        c, cell, least, where = autograd.field_clearance(plan, s, n, field, geometry)
        assert c.requires_grad and least.requires_grad and not cell.requires_grad and not where.requires_grad
        (c[0, :3].sum() + 8.0 * least.sum()).backward()
        torch.cuda.synchronize()
        assert c[0].tolist() == [3.5, 1.75, 13.5, float("inf")] and cell[0].tolist() == [0, 0, 2 * 6 + 2, -1]
        assert least.tolist() == [1.75] and where.tolist() == [[1, 0]]
        want = torch.tensor([[1.0, 2.0, 4.0, 0.0], [9.0, 18.0, 36.0, 0.0], [1.0, 2.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0]],
                            dtype=torch.float64, device="cuda")
        assert bool(torch.all(s.grad[0] == want))
        # through the minimum alone, with an outside value that IS the minimum: no gradient anywhere
        s2 = rows.clone().requires_grad_(True)
        _, _, least, where = autograd.field_clearance(plan, s2, n, field, geometry, outside_value=-1.0)
        least.sum().backward()
        torch.cuda.synchronize()
        assert least.tolist() == [-1.0] and where.tolist() == [[3, -1]] and not bool(s2.grad.any())
    finally:
        plan.close()


def test_field_built_on_the_device_from_nine_spheres_and_looked_up_again(gpu_ctx):
    """DESIGN.md section 11k's recipe: Plan.obstacle_clearance with the nodes of one (k, j) grid line as the rows of one path;
    its clearance output [nz ny][nx] IS the field.  field_clearance at a node with t = 0 then returns obstacle_clearance's
    value in bits (a + 0 (b - a) = a in every lerp); elsewhere the interpolant is within a cell's diagonal of the exact
    clearance (1-Lipschitz; a convex combination of corners no farther away), plus 1e-12 for rounding."""
    dims, spacing = (5, 4, 6), (0.25, 0.5, 1.0)
    geometry = api.FieldGeometry(fu.ORIGIN, spacing, dims, 1)
    nx, ny, nz = dims
    nodes = np.zeros((nz * ny, nx, 4))
    nodes[..., :3] = fu.node_coordinates(geometry).reshape(nz * ny, nx, 3)
    ob, off = _dev(fu.NINE_SPHERES), [0, 9]
    lines = api.Plan(gpu_ctx, np.arange(nz * ny + 1, dtype=np.int32))
    rng = np.random.default_rng(510)
    lo, hi = np.array(fu.ORIGIN), fu.upper_corner(fu.ORIGIN, spacing, dims)
    free = np.zeros((nz * ny, nx, 4))
    free[..., :3] = rng.uniform(lo, hi, (nz * ny, nx, 3))
    try:
        count = torch.full((nz * ny,), nx, dtype=torch.int32, device="cuda")
        field = torch.empty((nz * ny, nx), dtype=torch.float64, device="cuda")
        lines.obstacle_clearance(_dev(nodes), count, ob, off, clearance=field)
        exact_free = torch.empty((nz * ny, nx), dtype=torch.float64, device="cuda")
        lines.obstacle_clearance(_dev(free), count, ob, off, clearance=exact_free)
        fields = field.reshape(1, nz, ny, nx)
        assert fu.same_bits(fields.cpu().numpy()[0], fu.field_from_obstacles(fu.NINE_SPHERES, geometry))
        on = torch.empty_like(field)
        cell = torch.empty((nz * ny, nx), dtype=torch.int32, device="cuda")
        lines.field_clearance(_dev(nodes), count, fields, geometry, clearance=on, cell=cell)
        off_nodes = torch.empty_like(field)
        lines.field_clearance(_dev(free), count, fields, geometry, clearance=off_nodes)
        torch.cuda.synchronize()
        on, want, cell = on.cpu().numpy().reshape(nz, ny, nx), field.cpu().numpy().reshape(nz, ny, nx), cell.cpu().numpy()
        assert np.all(cell >= 0)
        assert fu.same_bits(on[:-1, :-1, :-1], want[:-1, :-1, :-1])              # every node with t = 0
        bound = np.sqrt(sum(h * h for h in spacing)) + 1e-12
        assert np.all(np.abs(on - want) <= bound)                                 # the upper faces: t = 1, a + (b - a)
        err = np.abs(off_nodes.cpu().numpy() - exact_free.cpu().numpy())
        print("FIELD GPU: nine spheres, max |interpolant - exact| off the nodes %.4f, bound %.4f" % (err.max(), bound))
        assert np.all(err <= bound) and err.max() > 1e-6
    finally:
        lines.close()


def _torch_field_stage(samples, n, fields, geometry, cap):
    """the torch composition: the same trilinear expression, the cell chosen as the step chooses it and detached"""
    o = torch.tensor(geometry.origin, dtype=torch.float64, device=samples.device)
    h = torch.tensor(geometry.spacing, dtype=torch.float64, device=samples.device)
    dims = torch.tensor(geometry.dims, dtype=torch.float64, device=samples.device)
    nx, ny, nz = geometry.dims
    u = (samples[..., :3] - o) / h
    inside = ((u >= 0.0) & (u <= dims - 1.0)).all(dim=-1)
    idx = torch.minimum(torch.where(inside[..., None], u, torch.zeros_like(u)).detach().floor(), dims - 2.0)
    t = u - idx
    i, j, k = (idx[..., a].long() for a in range(3))
    flat = fields.reshape(-1)
    v = [flat[((k + K) * ny + (j + J)) * nx + (i + I)] for K in (0, 1) for J in (0, 1) for I in (0, 1)]
    lerp = lambda a, b, x: a + x * (b - a)
    c00, c10 = lerp(v[0], v[1], t[..., 0]), lerp(v[2], v[3], t[..., 0])
    c01, c11 = lerp(v[4], v[5], t[..., 0]), lerp(v[6], v[7], t[..., 0])
    c = lerp(lerp(c00, c10, t[..., 1]), lerp(c01, c11, t[..., 1]), t[..., 2])
    valid = torch.arange(cap, device=samples.device)[None, :] < torch.clamp(n, max=cap)[:, None]
    cell = torch.where(valid & inside, (k * ny + j) * nx + i, torch.full_like(i, -1))
    return torch.where(valid & inside, c, torch.full_like(c, float("inf"))), cell, valid


def test_chain_solve_sample_field_clearance_hinge_loss(gpu_ctx):
    """fixed_values.grad and seg_times.grad of the hinge relu(R - clearance) through solve -> sample -> field_clearance on
    three 4-segment paths and the field of nine obstacles on a grid of half a metre, against the same chain with the torch
    trilinear composition in place of the step.

    The bound.  The two chains share the solve and the sampler (same kernels, same bits); they differ in what the clearance
    stage hands back.  That is checked first, entry by entry: an entry of dL/dsamples is g times a sum of eight corner values
    with bilinear weights over the spacing, and the two are held to 1e-13 of the sum of the absolute terms (fu.GRAD_RTOL, the
    bound tests/test_field_host.py holds the harness to torch with).  This is a relative error rho = 1e-13 of every row's
    contribution, and the final gradients are held to rho times the composition's own gradient norm, per path, as
    tests/test_gpu_obstacle.py::test_chain_solve_sample_obstacle_clearance_hinge_loss does it.  The figures are printed.

    Measured on an MI355X: dL/dsamples 6.7e-16 under a largest bound of 8.2e-13; fixed_values.grad
    3.1e-14 .. 6.3e-14 under 8.2e-13 .. 1.0e-12; seg_times.grad 1.3e-14 .. 1.2e-13 under 2.3e-13 .. 3.6e-13."""
    batch, obstacles, geometry, field = fu.chain_batch()
    cap, dt, R = fu.CHAIN_CAPACITY, fu.CHAIN_DT, fu.CHAIN_RADIUS
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    so = np.asarray(batch.seg_offsets, dtype=np.int64)
    P = batch.n_paths
    assert P == 3 and np.all(np.diff(so) == 4) and obstacles.shape == (9, 4)
    v0 = so[:-1] + np.arange(P)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    mask, fl = _dev(batch.fixed_mask), _dev(field)
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
            c, cell, least, where = autograd.field_clearance(plan, samples, n, fl, geometry, status=status)
            c.retain_grad()
            return torch.relu(R - c).sum(), dict(c=c, cell=cell, least=least, where=where)   # (no mask: +inf behind the last row)

        def torch_stage(samples, n, status):
            c, cell, valid = _torch_field_stage(samples, n, fl, geometry, cap)
            c.retain_grad()
            return (torch.relu(R - c) * valid).sum(), dict(c=c, cell=cell)

        k, r = chain(kernel_stage), chain(torch_stage)
        assert k["c"].requires_grad and not k["cell"].requires_grad
        k["loss"].backward()
        r["loss"].backward()
        torch.cuda.synchronize()
        n = k["n"].cpu().numpy()
        assert bool(torch.all(k["status"] > 0))
        ck, cr = k["c"].detach().cpu().numpy(), r["c"].detach().cpu().numpy()
        qk, qr = k["cell"].cpu().numpy(), r["cell"].cpu().numpy()
        live = np.arange(cap)[None, :] < np.minimum(n, cap)[:, None]
        assert np.all(qk[live] >= 0) and np.all(qk[~live] == -1) and np.all(ck[~live] == np.inf)      # the grid holds every row
        assert np.array_equal(qk, qr) and np.max(np.abs(ck[live] - cr[live])) <= 1e-13
        assert np.array_equal(k["least"].detach().cpu().numpy(), ck.min(axis=1))
        assert np.array_equal(k["where"].cpu().numpy()[:, 0], ck.argmin(axis=1))
        active = live & (ck < R)
        print("FIELD GPU CHAIN: rows per path %s, rows inside the hinge per path %s, least clearance %.3f, cells in use %d"
              % (np.minimum(n, cap).tolist(), active.sum(axis=1).tolist(), ck[live].min(), len(np.unique(qk[live]))))
        assert np.all(active.sum(axis=1) >= 5)                                     # the loss is alive on every path
        # the stage's own gradient, entry by entry, within 1e-13 of the sum of its absolute terms
        Gs_k, Gs_r = k["samples"].grad.cpu().numpy(), r["samples"].grad.cpu().numpy()
        arr = dict(samples=k["samples"].detach().cpu().numpy(), n=n.astype(np.int32), status=np.ones(P, dtype=np.int32),
                   fields=field, origin=geometry.origin, spacing=geometry.spacing, path_field=None,
                   upstream=k["c"].grad.cpu().numpy(), outside_value=np.inf)
        scale = fu.gradient_scale(arr, fu.followed(arr, qk))
        diff = np.abs(Gs_k - Gs_r)
        print("FIELD GPU CHAIN: dL/dsamples max |diff| %.2e, largest bound %.2e, worst (diff - bound) %.2e"
              % (diff.max(), fu.GRAD_RTOL * scale.max(), np.max(diff - fu.GRAD_RTOL * scale)))
        assert fu.grads_agree(Gs_k, Gs_r, scale)
        assert not Gs_k[..., 3].any() and not Gs_k[~live].any() and np.any(Gs_k[active] != 0.0)
    finally:
        plan.close()
    rho = fu.GRAD_RTOL
    gfk, gfr, gtk, gtr = (x.grad.cpu().numpy() for x in (k["fv"], r["fv"], k["times"], r["times"]))
    worst = []
    for p in range(P):
        vs, ss = slice(v0[p], v0[p] + 5), slice(so[p], so[p + 1])
        ef, et = np.abs(gfk[vs] - gfr[vs]).max(), np.abs(gtk[ss] - gtr[ss]).max()
        nf, nt = np.linalg.norm(gfr[vs]), np.linalg.norm(gtr[ss])
        print("FIELD GPU CHAIN path %d: fixed_values.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e); "
              "seg_times.grad max |diff| %.2e (bound %.2e, ||grad|| %.2e)" % (p, ef, rho * nf, nf, et, rho * nt, nt))
        assert nf > 0 and nt > 0 and np.all(np.isfinite(gfk[vs])) and np.all(np.isfinite(gtk[ss]))
        worst.append((ef - rho * nf, et - rho * nt))
    assert all(f <= 0.0 and t <= 0.0 for f, t in worst), worst


TIE_ROWS = (5, 37, 70, 200, 260)      # at capacity 264: lanes 5 and 37 of wavefront 0, wavefronts 1 and 3, lane 4's second row


def _tie_case(keep):
    """A (4, 3, 2) grid of unit spacing at the origin whose field depends on x alone: 1, 1, 3, 3 on the four node planes, so it
    is the constant 1 on the cells with i = 0, the constant 3 on those with i = 2 and 1 + 2 t between.  A path of 261 rows:
    the rows of `keep` in the cells (0, 0, 0) and (0, 1, 0) in turn, the other rows of TIE_ROWS where the field is 3, the rest
    at 1.25 .. 3 -- every operation of the lookup exact.  Path 1 is dead (NaN rows); path 2 names no grid: every row +inf."""
    m = 261
    fields = np.zeros((1, 2, 3, 4))
    fields[...] = np.array([1.0, 1.0, 3.0, 3.0])
    rows = np.zeros((m, 4))
    rows[:, 0] = 1.125 + 0.125 * (np.arange(m) % 8)
    rows[:, 1] = 0.25 + 0.0625 * (np.arange(m) % 24)
    rows[:, 2] = 0.5
    for k, r in enumerate(TIE_ROWS):
        rows[r, :3] = [0.5, 0.5 + (k % 2), 0.25] if r in keep else [2.5, 0.5, 0.25]
    dead = dict(fu.path(np.full((m, 4), np.nan)), status=0)
    return fu.case([fu.path(rows), dead, fu.path(rows)], fields, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), path_field=[0, 0, -1])


@pytest.mark.parametrize("first", range(len(TIE_ROWS)))
def test_rows_that_tie_for_the_path_minimum_give_the_lowest_row(gpu_ctx, harness, first):
    """the same double on several rows of one path -- in one wavefront, across wavefronts, in a lane's second row: the lowest
    tied row is the argmin, as in the harness"""
    keep = TIE_ROWS[first:]
    arr = fu.batch_arrays(_tie_case(keep))
    assert arr["samples"].shape[1] == 264
    got, want = _run(gpu_ctx, arr), fu.run_harness(harness, arr)
    tied = np.flatnonzero(want["clearance"][0] == want["min_clearance"][0])
    assert tied.tolist() == list(keep) and want["min_clearance"][0] == 1.0 and np.all(want["clearance"][0, :261] >= 1.0)
    _same(got, want, "tie kept on rows %s" % (keep,))
    assert fu.same_bits(got["min_clearance"], [1.0, np.inf, np.inf])
    cell = 4 * (TIE_ROWS.index(keep[0]) % 2)                # (0, j, 0) of grid 0 in a row of nx = 4
    assert got["argmin"].tolist() == [[keep[0], cell], [-1, -1], [-1, -1]]

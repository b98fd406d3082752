"""mrs_tg_field_from_occupancy on the GPU (edt_x_kernel, edt_y_kernel, edt_z_kernel) and
Context.field_from_occupancy on top of it: every case of tests/test_edt_host.py against the CPU harness bit for bit, the output
between guard regions and the occupancy unchanged; two calls, a large grid followed by a small one, another stream; the argument
checks and the empty call; and the seam to the clearance steps -- Plan.field_clearance on the device-built field against the
same on the brute-force field, and the device-built field against section 11k's device recipe over the occupied nodes.  Only
well-formed inputs go to the device: nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import edt_util as eu
from tests import field_util as fu

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 96              # doubles in front of and behind the output
INVALID_ARG = -1
KERNELS = ["edt_x_kernel", "edt_y_kernel", "edt_z_kernel"]


def _guarded(shape):
    n = int(np.prod(shape))
    full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return full, full[GUARD:GUARD + n].view(shape)


def _run(ctx, c, calls=1):
    """the case on the device -> [F][nz][ny][nx] (a list of them for calls > 1); guards and occupancy checked"""
    occ = torch.from_numpy(c["occupancy"]).cuda()
    g = eu.geometry_of(c)
    out = []
    for _ in range(calls):
        full, view = _guarded(g.fields_shape())
        got = ctx.field_from_occupancy(occ, g, z_scale=c["z_scale"], max_distance=c["max_distance"], signed=c["signed"], out=view)
        torch.cuda.synchronize()
        assert got is view
        host = full.cpu().numpy()
        assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), "a neighbour of the output was written"
        out.append(host[GUARD:-GUARD].reshape(g.fields_shape()).copy())
    assert np.array_equal(occ.cpu().numpy(), c["occupancy"]), "the occupancy was written"
    return out if calls > 1 else out[0]


@pytest.fixture(scope="module")
def cases():
    return list(eu.all_cases())


@pytest.fixture(scope="module")
def harness_results(tmp_path_factory, cases):
    """the CPU harness on every case, once for the module"""
    return eu.run_harness(eu.build_harness(tmp_path_factory.mktemp("edt_gpu")), cases)


def _pick(cases, results, dims, spacing=eu.SPACINGS[1], z_scale=0.5, cap=np.inf, signed=True):
    for c, r in zip(cases, results):
        if (c["dims"], c["spacing"], c["z_scale"], c["max_distance"], c["signed"]) == (dims, spacing, z_scale, cap, signed):
            return c, r
    raise KeyError(dims)


def test_capability_bit_timing_id_and_kernel_names(gpu_ctx, cases, harness_results):
    assert api.capabilities() & api.CAP_FIELD_FROM_OCCUPANCY and api.CAP_FIELD_FROM_OCCUPANCY == 524288
    assert api.KERNEL_FIELD_FROM_OCCUPANCY == 41
    try:
        gpu_ctx.set_profiling(True)
        for signed in (True, False):
            c, want = _pick(cases, harness_results, (5, 4, 70), signed=signed)
            api.kernel_trace_reset()
            got = _run(gpu_ctx, c)
            assert api.kernel_trace() == KERNELS
            assert gpu_ctx.last_kernel_ms(api.KERNEL_FIELD_FROM_OCCUPANCY) > 0.0
            assert eu.SAME_BITS(got, want)
    finally:
        gpu_ctx.set_profiling(False)


def test_every_cpu_case_is_the_harness_in_bits(gpu_ctx, cases, harness_results):
    voxels = 0
    for c, want in zip(cases, harness_results):
        got = _run(gpu_ctx, c)
        assert eu.SAME_BITS(got, want), (eu.case_name(c), [n for n, a, b in zip(c["names"], got, want) if not eu.SAME_BITS(a, b)])
        voxels += got.size
    assert len(cases) == 200 and voxels > 2_000_000


def test_two_calls_give_the_same_bits(gpu_ctx, cases, harness_results):
    for dims, signed in (((5, 4, 70), True), ((130, 3, 2), False), (eu.SPARSE_DIMS, True)):
        c, want = _pick(cases, harness_results, dims, signed=signed)
        a, b = _run(gpu_ctx, c, calls=2)
        assert eu.SAME_BITS(a, b) and eu.SAME_BITS(a, want), dims


def test_a_large_grid_then_a_small_one_gives_the_same_bits(gpu_ctx, cases, harness_results):
    """nothing of a call outlives it: a small grid behind a large one, and back"""
    large, want_large = _pick(cases, harness_results, eu.SPARSE_DIMS, cap=1.0)
    small, want_small = _pick(cases, harness_results, (2, 2, 2), cap=1.0)
    middle, want_middle = _pick(cases, harness_results, (65, 2, 3), cap=1.0)
    for c, want in ((large, want_large), (small, want_small), (middle, want_middle), (large, want_large), (small, want_small)):
        assert eu.SAME_BITS(_run(gpu_ctx, c), want), eu.case_name(c)


def test_another_stream(gpu_ctx, cases, harness_results):
    c, want = _pick(cases, harness_results, (65, 2, 3))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    try:
        with torch.cuda.stream(s):
            gpu_ctx.use_torch_stream()
            got = _run(gpu_ctx, c)
    finally:
        torch.cuda.synchronize()
        gpu_ctx.use_torch_stream()
    assert eu.SAME_BITS(got, want)


def test_arguments_are_checked_before_any_launch_and_the_empty_call(gpu_ctx):
    L = api.load_library()
    dims, spacing = (5, 4, 7), (0.25, 0.5, 1.0)
    voxels = 2 * 5 * 4 * 7
    occ = torch.zeros((2, 7, 4, 5), dtype=torch.uint8, device="cuda")
    occ[0, 3, 2, 2] = 1
    out = torch.full((2, 7, 4, 5), SENTINEL, dtype=torch.float64, device="cuda")
    both = torch.zeros((voxels * 9 + 64,), dtype=torch.uint8, device="cuda")     # room for an output that overlaps its input
    ptr = api._t_ptr
    inf, nan = float("inf"), float("nan")

    def geo(**kw):
        a = dict(origin=eu.ORIGIN, spacing=spacing, dims=dims, n_fields=2)
        a.update(kw)
        return api.C.byref(api.FieldGeometry(**a).as_struct())

    def at(t, nbytes):
        return api.C.c_void_p(t.data_ptr() + nbytes)

    def call(ctx=gpu_ctx._h, occupancy=ptr(occ), geometry=geo(), z_scale=1.0, max_distance=inf, flags=api.FIELD_SIGNED,
             fields=ptr(out)):
        return L.mrs_tg_field_from_occupancy(ctx, occupancy, geometry, z_scale, max_distance, flags, fields)

    def refused(rc):
        return rc == INVALID_ARG and len(L.mrs_tg_last_error(gpu_ctx._h)) > 0

    api.kernel_trace_reset()
    assert call(ctx=None) == INVALID_ARG and len(L.mrs_tg_last_error(None)) > 0
    first = (both.data_ptr() + 7) // 8 * 8 - both.data_ptr()     # an 8-byte aligned place in `both`
    for bad in (dict(geometry=None), dict(occupancy=None), dict(fields=None), dict(geometry=geo(n_fields=-1)),
                dict(geometry=geo(dims=(1, 4, 7))), dict(geometry=geo(dims=(5, 0, 7))), dict(geometry=geo(dims=(5, 4, -7))),
                dict(geometry=geo(spacing=(0.0, 0.5, 1.0))), dict(geometry=geo(spacing=(0.25, -0.5, 1.0))),
                dict(geometry=geo(spacing=(0.25, 0.5, nan))), dict(geometry=geo(spacing=(inf, 0.5, 1.0))),
                dict(geometry=geo(origin=(nan, 0.0, 0.0))), dict(geometry=geo(origin=(0.0, 0.0, -inf))),
                # a dim above the cap, on every axis
                dict(geometry=geo(dims=(api.FIELD_MAX_DIM + 1, 2, 2), n_fields=1)), dict(geometry=geo(dims=(2, 1025, 2), n_fields=1)),
                dict(geometry=geo(dims=(2, 2, 4096), n_fields=1)),
                # more voxels than 2^31 - 1 with every dim at the cap, with the small real buffers, which must not be touched
                dict(geometry=geo(dims=(1024, 1024, 1024), n_fields=2)), dict(geometry=geo(dims=(2, 2, 2), n_fields=2 ** 28)),
                dict(geometry=geo(dims=(1024, 1024, 1024), n_fields=2 ** 31 - 1)),
                dict(z_scale=0.0), dict(z_scale=-1.0), dict(z_scale=nan), dict(z_scale=inf),
                dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=nan), dict(max_distance=-inf),
                dict(flags=2), dict(flags=3), dict(flags=-1), dict(flags=1 << 30),
                dict(fields=at(out, 4)),
                # the output over its input: the same start, the input inside the output, the output's end on the input's start
                dict(occupancy=at(both, first), fields=at(both, first)), dict(occupancy=at(both, first + 8 * voxels - 1), fields=at(both, first)),
                dict(occupancy=at(both, first), fields=at(both, first + (voxels - 1) // 8 * 8))):
        assert refused(call(**bad)), bad
    assert b"overlaps" in L.mrs_tg_last_error(gpu_ctx._h)
    assert api.kernel_trace() == []
    # no grids: a success without a launch, whatever the pointers
    assert call(geometry=geo(n_fields=0)) == 0 and call(geometry=geo(n_fields=0), occupancy=None, fields=None) == 0
    assert api.kernel_trace() == []
    torch.cuda.synchronize()
    assert bool(torch.all(out == SENTINEL)) and not bool(both.any())
    g0 = api.FieldGeometry(eu.ORIGIN, spacing, dims, 0)
    empty = gpu_ctx.field_from_occupancy(torch.zeros(g0.fields_shape(), dtype=torch.uint8, device="cuda"), g0)
    assert tuple(empty.shape) == (0, 7, 4, 5) and empty.dtype == torch.float64 and api.kernel_trace() == []
    # an output that touches its input without overlapping it is taken
    assert call(occupancy=at(both, first + 8 * voxels), fields=at(both, first)) == 0
    torch.cuda.synchronize()
    assert api.kernel_trace() == KERNELS
    # the Python layer: dtype, device, contiguity and shape of both tensors, the geometry, the scalars
    g = api.FieldGeometry(eu.ORIGIN, spacing, dims, 2)
    for kw in (dict(occupancy=occ.cpu()), dict(occupancy=occ.bool()), dict(occupancy=occ.double()), dict(occupancy=occ[:1]),
               dict(occupancy=occ.transpose(2, 3)), dict(occupancy=occ.transpose(2, 3).contiguous()), dict(out=out.cpu()),
               dict(out=out.float()), dict(out=out[:1]), dict(out=out[..., :4]), dict(geometry=None),
               dict(geometry=api.FieldGeometry(eu.ORIGIN, spacing, (7, 4, 5), 2)), dict(z_scale=0.0), dict(max_distance=nan),
               dict(max_distance=0.0)):
        args = dict(occupancy=occ, geometry=g, out=out)
        args.update(kw)
        with pytest.raises(ValueError):
            gpu_ctx.field_from_occupancy(**args)
    api.kernel_trace_reset()
    got = gpu_ctx.field_from_occupancy(occ, g, max_distance=1.0)
    torch.cuda.synchronize()
    assert api.kernel_trace() == KERNELS and tuple(got.shape) == (2, 7, 4, 5)
    host = got.cpu().numpy()
    assert host[0, 3, 2, 2] == -0.25 and host[0, 3, 2, 3] == 0.25 and host[0, 3, 3, 2] == 0.5 and host[0, 0, 0, 0] == 1.0
    assert np.all(host[1] == 1.0)


def _seam_occupancy(geometry, seed):
    nx, ny, nz = geometry.dims
    return (np.random.default_rng(seed).random((1, nz, ny, nx)) < 0.02).astype(np.uint8)


def test_seam_field_clearance_on_the_device_built_field(gpu_ctx):
    """three 4-segment paths, solve -> sample -> field_clearance: on the field built on the device from an occupancy grid and
    on the brute-force field of tests/edt_util.py, the same bits in clearance, cell, gradient and minimum"""
    batch, _, geometry, _ = fu.chain_batch()
    cap, dt = fu.CHAIN_CAPACITY, fu.CHAIN_DT
    occupancy = _seam_occupancy(geometry, 11)
    assert 50 < occupancy.sum() < 300
    c = dict(dims=geometry.dims, spacing=geometry.spacing, z_scale=1.0, max_distance=3.0, signed=True, occupancy=occupancy,
             names=["seam"])
    want_field = eu.brute_force(c)
    built = gpu_ctx.field_from_occupancy(torch.from_numpy(occupancy).cuda(), geometry, max_distance=3.0)
    torch.cuda.synchronize()
    assert eu.SAME_BITS(built.cpu().numpy(), want_field) and np.all(np.isfinite(want_field))
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    P = batch.n_paths
    assert P == 3 and np.all(np.diff(np.asarray(batch.seg_offsets)) == 4)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        coeffs, _, status = autograd.solve(plan, dev(batch.fixed_mask), dev(batch.fixed_values), dev(times0))
        samples, n = autograd.sample(plan, coeffs, dev(times0), dt, cap, status)
        samples, n = samples.detach().contiguous(), n.contiguous()
        results = []
        for field in (built, dev(want_field)):
            o = dict(clearance=torch.empty((P, cap), dtype=torch.float64, device="cuda"),
                     cell=torch.empty((P, cap), dtype=torch.int32, device="cuda"),
                     gradient=torch.empty((P, cap, 4), dtype=torch.float64, device="cuda"),
                     min_clearance=torch.empty((P,), dtype=torch.float64, device="cuda"),
                     argmin=torch.empty((P, 2), dtype=torch.int32, device="cuda"))
            plan.field_clearance(samples, n, field, geometry, status=status, outside_value=3.0, **o)
            torch.cuda.synchronize()
            results.append({k: v.cpu().numpy() for k, v in o.items()})
        a, b = results
        for k in ("clearance", "gradient", "min_clearance"):
            assert eu.SAME_BITS(a[k], b[k]), k
        assert np.array_equal(a["cell"], b["cell"]) and np.array_equal(a["argmin"], b["argmin"])
        # the comparison is about something: the grid holds every live row of the three paths, each in cells of its own
        live = a["cell"] >= 0
        rows = np.minimum(n.cpu().numpy(), cap)
        assert np.all(rows > 0) and np.array_equal(live, np.arange(cap)[None, :] < rows[:, None])
        assert np.all(np.isfinite(a["clearance"][live])) and np.any(a["gradient"][live] != 0.0)
        assert np.all(np.isfinite(a["min_clearance"])) and len(np.unique(a["cell"][live])) >= P
    finally:
        plan.close()


@pytest.mark.parametrize("z_scale", eu.Z_SCALES)
def test_seam_device_built_field_is_the_device_recipe_over_the_occupied_nodes(gpu_ctx, z_scale):
    """DESIGN.md section 11k's recipe -- Plan.obstacle_clearance with the nodes of one grid line as the rows of one path, the
    occupied nodes as points of radius 0 -- on the power-of-two geometry of the chain test, where every coordinate, square and
    sum is exact: the unsigned field without a cap, in bits"""
    _, _, geometry, _ = fu.chain_batch()
    assert geometry.spacing == (0.5, 0.5, 0.5)
    nx, ny, nz = geometry.dims
    occupancy = _seam_occupancy(geometry, 12)
    built = gpu_ctx.field_from_occupancy(torch.from_numpy(occupancy).cuda(), geometry, z_scale=z_scale, signed=False)
    coordinates = fu.node_coordinates(geometry)
    nodes = np.zeros((nz * ny, nx, 4))
    nodes[..., :3] = coordinates.reshape(nz * ny, nx, 3)
    points = np.zeros((int(occupancy.sum()), 4))
    points[:, :3] = coordinates[occupancy[0] != 0]
    lines = api.Plan(gpu_ctx, np.arange(nz * ny + 1, dtype=np.int32))
    try:
        count = torch.full((nz * ny,), nx, dtype=torch.int32, device="cuda")
        recipe = torch.empty((nz * ny, nx), dtype=torch.float64, device="cuda")
        lines.obstacle_clearance(torch.from_numpy(nodes).cuda(), count, torch.from_numpy(points).cuda(), [0, len(points)],
                                 z_scale=z_scale, clearance=recipe)
        torch.cuda.synchronize()
        assert eu.SAME_BITS(built.cpu().numpy()[0], recipe.cpu().numpy().reshape(nz, ny, nx))
        assert np.count_nonzero(built.cpu().numpy() == 0.0) == len(points)
    finally:
        lines.close()

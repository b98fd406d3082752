"""mrs_tg_field_update_region on the GPU (edt_region_x_kernel, edt_region_y_kernel, edt_region_z_kernel)
and Context.field_update_region on top of it: every case of tests/test_edt_region_host.py against the CPU harness bit for bit,
the field between guard regions and filled with a sentinel outside the core, the workspace between guard regions, the
occupancy unchanged; the chain build -> change a box on the device -> update against the rebuild and the brute force; the
kernels of both routes and their timing; two calls, a large window followed by a small one, another stream; the argument
checks; and the seam to the clearance step.  Only well-formed inputs go to the device: nothing provokes a fault."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, autograd
from tests import edt_region_util as ru
from tests import edt_util as eu
from tests import field_util as fu

pytestmark = pytest.mark.gpu

SENTINEL = ru.SENTINEL
GUARD = 96              # doubles in front of and behind the field and the workspace
INVALID_ARG = -1
REGION_KERNELS = ["edt_region_x_kernel", "edt_region_y_kernel", "edt_region_z_kernel"]
FULL_KERNELS = ["edt_x_kernel", "edt_y_kernel", "edt_z_kernel"]


def _guarded(n):
    full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    return full, full[GUARD:GUARD + n]


def _guards_hold(full, what):
    host = full.cpu().numpy()
    assert np.all(host[:GUARD] == SENTINEL) and np.all(host[-GUARD:] == SENTINEL), "a neighbour of the %s was written" % what


def _run(ctx, rc, start, own_workspace=True):
    """the region case on the device from the field `start` [F][nz][ny][nx] -> the field afterwards; the guards of the field and
    of the workspace and the occupancy checked"""
    c = rc["new"]
    occ = torch.from_numpy(c["occupancy"]).cuda()
    g = eu.geometry_of(c)
    info = ru.query(rc)
    full, flat = _guarded(start.size)
    view = flat.view(g.fields_shape())
    view.copy_(torch.from_numpy(np.ascontiguousarray(start)))
    ws_full, ws = _guarded(info["workspace_bytes"] // 8)
    got = ctx.field_update_region(occ, view, g, rc["lo"], rc["hi"], field=rc["field"], z_scale=c["z_scale"],
                                  max_distance=c["max_distance"], signed=c["signed"],
                                  workspace=ws if own_workspace and info["workspace_bytes"] else None)
    torch.cuda.synchronize()
    assert got is view
    _guards_hold(full, "field")
    _guards_hold(ws_full, "workspace")
    assert np.array_equal(occ.cpu().numpy(), c["occupancy"]), "the occupancy was written"
    return full.cpu().numpy()[GUARD:-GUARD].reshape(g.fields_shape()).copy()


@pytest.fixture(scope="module")
def cases():
    return list(ru.all_cases())


@pytest.fixture(scope="module")
def harness_results(tmp_path_factory, cases):
    """per case (the old field, the harness's (info, updated, marked)): the old fields from the CPU harness of the full
    transform, once per geometry, mode and cap; the CPU harness of the update on every case, once for the module"""
    tmp = tmp_path_factory.mktemp("edt_region_gpu")
    olds, keys = {}, []
    for rc in cases:
        c = rc["old"]
        key = (c["dims"], c["spacing"], c["z_scale"], c["max_distance"], c["signed"])
        olds.setdefault(key, c)
        keys.append(key)
    fields = dict(zip(olds, eu.run_harness(eu.build_harness(tmp), list(olds.values()))))
    old_fields = [fields[k] for k in keys]
    return list(zip(old_fields, ru.run_harness(ru.build_harness(tmp), cases, old_fields)))


def _pick(cases, results, dims, box, spacing=eu.SPACINGS[1], cap=1.0, signed=True):
    for rc, r in zip(cases, results):
        c = rc["new"]
        if (c["dims"], rc["box"], c["spacing"], c["max_distance"], c["signed"]) == (dims, box, spacing, cap, signed):
            return rc, r
    raise KeyError((dims, box))


def test_every_cpu_case_is_the_harness_in_bits_and_only_the_core_is_written(gpu_ctx, cases, harness_results):
    windows = changed = 0
    for rc, (old_field, (info, updated, marked)) in zip(cases, harness_results):
        name = ru.case_name(rc)
        assert info == ru.query(rc), name
        core = ru.core_mask(info, rc["new"]["dims"], old_field.shape[0], rc["field"])
        # the old field on the core, the sentinel everywhere else: the core becomes the new field, the sentinels survive
        got = _run(gpu_ctx, rc, np.where(core, old_field, SENTINEL))
        assert eu.SAME_BITS(got[core], updated[core]), name
        assert np.all(got[~core] == SENTINEL), name + ": an element outside the core was written"
        assert eu.SAME_BITS(got, marked), name
        windows += 1 - info["whole_grid"]
        changed += int((old_field.view(np.int64) != updated.view(np.int64)).sum())
    assert len(cases) == 438 and windows > 300 and changed > 1000


@pytest.mark.parametrize("signed", (True, False))
def test_chain_build_change_a_box_on_the_device_update(gpu_ctx, signed):
    """field_from_occupancy(old), a box rewritten on the device, field_update_region: the field of field_from_occupancy(new) and
    the brute force of the new occupancy"""
    dims, (spacing, z_scale), cap = eu.SPARSE_DIMS, ru.GEOMETRIES[1], 1.0
    lo, hi = (12, 11, 14), (19, 17, 20)
    old = ru.old_grid(dims, 21)
    g = api.FieldGeometry(eu.ORIGIN, spacing, dims, 1)
    occ = torch.from_numpy(old[None].copy()).cuda()
    field = gpu_ctx.field_from_occupancy(occ, g, z_scale=z_scale, max_distance=cap, signed=signed)
    before = field.clone()
    patch = torch.from_numpy(ru.changed_occupancy(old, lo, hi, 22)[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1].copy()).cuda()
    occ[0, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = patch
    api.kernel_trace_reset()
    got = gpu_ctx.field_update_region(occ, field, g, lo, hi, z_scale=z_scale, max_distance=cap, signed=signed)
    assert got is field and api.kernel_trace() == REGION_KERNELS
    rebuilt = gpu_ctx.field_from_occupancy(occ, g, z_scale=z_scale, max_distance=cap, signed=signed)
    torch.cuda.synchronize()
    new = occ.cpu().numpy()
    assert np.array_equal(new[0], ru.changed_occupancy(old, lo, hi, 22))
    want = eu.brute_force(eu.stacked(dims, spacing, z_scale, cap, signed, {"new": new[0]}))
    assert eu.SAME_BITS(field.cpu().numpy(), rebuilt.cpu().numpy()) and eu.SAME_BITS(field.cpu().numpy(), want)
    assert int((before != field).sum()) > 100


def test_capability_bit_kernel_names_and_timing_of_both_routes(gpu_ctx, cases, harness_results):
    assert api.capabilities() & api.CAP_FIELD_UPDATE_REGION and api.CAP_FIELD_UPDATE_REGION == 1048576
    try:
        gpu_ctx.set_profiling(True)
        for box, kernels in (("middle_voxel", REGION_KERNELS), ("whole_grid", FULL_KERNELS)):
            rc, (old_field, (info, updated, _)) = _pick(cases, harness_results, (5, 4, 70), box)
            assert info["whole_grid"] == (box == "whole_grid")
            api.kernel_trace_reset()
            got = _run(gpu_ctx, rc, old_field)
            assert api.kernel_trace() == kernels
            assert gpu_ctx.last_kernel_ms(api.KERNEL_FIELD_FROM_OCCUPANCY) > 0.0
            assert eu.SAME_BITS(got, updated)
    finally:
        gpu_ctx.set_profiling(False)


def test_two_calls_a_large_window_then_a_small_one_and_a_workspace_of_the_layers(gpu_ctx, cases, harness_results):
    """nothing of a call outlives it"""
    large = _pick(cases, harness_results, eu.SPARSE_DIMS, "face_x0")
    small = _pick(cases, harness_results, (5, 4, 70), "middle_voxel")
    straddle = _pick(cases, harness_results, (130, 3, 2), "straddle_64_128", signed=False)
    whole = _pick(cases, harness_results, (65, 2, 3), "whole_grid")
    for rc, (old_field, (info, updated, _)) in (large, large, small, straddle, whole, large, small):
        assert eu.SAME_BITS(_run(gpu_ctx, rc, old_field), updated), ru.case_name(rc)
    # the workspace the Python layer allocates when none is given
    rc, (old_field, (info, updated, _)) = large
    assert eu.SAME_BITS(_run(gpu_ctx, rc, old_field, own_workspace=False), updated)
    # an update of an up-to-date field changes nothing
    assert eu.SAME_BITS(_run(gpu_ctx, rc, updated), updated)


def test_another_stream(gpu_ctx, cases, harness_results):
    rc, (old_field, (info, updated, _)) = _pick(cases, harness_results, (2, 65, 3), "corner_5")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    try:
        with torch.cuda.stream(s):
            gpu_ctx.use_torch_stream()
            got = _run(gpu_ctx, rc, old_field)
    finally:
        torch.cuda.synchronize()
        gpu_ctx.use_torch_stream()
    assert eu.SAME_BITS(got, updated) and not info["whole_grid"]


def test_arguments_are_checked_before_any_launch(gpu_ctx):
    L = api.load_library()
    dims, spacing = (5, 4, 7), (0.25, 0.5, 1.0)
    voxels = 2 * 5 * 4 * 7
    occ = torch.zeros((2, 7, 4, 5), dtype=torch.uint8, device="cuda")
    occ[1, 3, 2, 2] = 1
    fields = torch.full((2, 7, 4, 5), SENTINEL, dtype=torch.float64, device="cuda")
    g = api.FieldGeometry(eu.ORIGIN, spacing, dims, 2)
    need = api.field_update_query(g, (2, 2, 3), (2, 2, 3), field=1, max_distance=1.0)["workspace_bytes"]
    assert need > 0
    ws = torch.full((need // 8 + 2,), SENTINEL, dtype=torch.float64, device="cuda")
    both = torch.zeros((voxels * 9 + need + 64,), dtype=torch.uint8, device="cuda")     # room for arrays that overlap
    ptr = api._t_ptr
    inf, nan = float("inf"), float("nan")

    def geo(**kw):
        a = dict(origin=eu.ORIGIN, spacing=spacing, dims=dims, n_fields=2)
        a.update(kw)
        return api.C.byref(api.FieldGeometry(**a).as_struct())

    def region(field=1, lo=(2, 2, 3), hi=(2, 2, 3)):
        r = api.FieldRegion()
        r.field, r.lo[:], r.hi[:] = field, lo, hi
        return api.C.byref(r)

    def at(t, nbytes):
        return api.C.c_void_p(t.data_ptr() + nbytes)

    def call(ctx=gpu_ctx._h, occupancy=ptr(occ), geometry=geo(), z_scale=1.0, max_distance=1.0, flags=api.FIELD_SIGNED,
             reg=region(), workspace=ptr(ws), workspace_bytes=need, field=ptr(fields)):
        return L.mrs_tg_field_update_region(ctx, occupancy, geometry, z_scale, max_distance, flags, reg, workspace, workspace_bytes,
                                            field)

    def refused(rc):
        return rc == INVALID_ARG and len(L.mrs_tg_last_error(gpu_ctx._h)) > 0

    api.kernel_trace_reset()
    assert call(ctx=None) == INVALID_ARG and len(L.mrs_tg_last_error(None)) > 0
    first = (both.data_ptr() + 7) // 8 * 8 - both.data_ptr()     # an 8-byte aligned place in `both`
    for bad in (dict(geometry=None), dict(occupancy=None), dict(field=None), dict(reg=None),
                # what mrs_tg_field_from_occupancy refuses
                dict(geometry=geo(n_fields=-1)), dict(geometry=geo(dims=(1, 4, 7))), dict(geometry=geo(dims=(5, 4, -7))),
                dict(geometry=geo(spacing=(0.0, 0.5, 1.0))), dict(geometry=geo(spacing=(0.25, 0.5, nan))),
                dict(geometry=geo(origin=(nan, 0.0, 0.0))), dict(geometry=geo(dims=(api.FIELD_MAX_DIM + 1, 4, 7), n_fields=1), reg=region(0)),
                dict(geometry=geo(dims=(1024, 1024, 1024), n_fields=2)),
                dict(z_scale=0.0), dict(z_scale=nan), dict(z_scale=inf), dict(max_distance=0.0), dict(max_distance=nan),
                dict(max_distance=-inf), dict(flags=2), dict(flags=-1), dict(field=at(fields, 4)),
                dict(occupancy=at(both, first), field=at(both, first)),
                dict(occupancy=at(both, first + 8 * voxels - 1), field=at(both, first)),
                # no grid to update, and the region
                dict(geometry=geo(n_fields=0)), dict(reg=region(field=2)), dict(reg=region(field=-1)),
                dict(reg=region(lo=(3, 2, 3))), dict(reg=region(lo=(2, 3, 3))), dict(reg=region(lo=(2, 2, 4))),
                dict(reg=region(lo=(-1, 2, 3))), dict(reg=region(hi=(5, 2, 3))), dict(reg=region(hi=(2, 4, 3))),
                dict(reg=region(hi=(2, 2, 7))),
                # the workspace: missing, misaligned, too small, over the occupancy, over the field (its end on the field's start)
                dict(workspace=None), dict(workspace=at(ws, 4)), dict(workspace_bytes=need - 8), dict(workspace_bytes=0),
                dict(workspace_bytes=-8),
                dict(occupancy=at(both, first + need - 1), workspace=at(both, first), field=at(both, first + need + voxels + 8)),
                dict(occupancy=at(both, first), workspace=at(both, first + 8 * voxels + need), field=at(both, first + need + 8)),
                dict(occupancy=at(both, first + 8 * voxels + need), workspace=at(both, first), field=at(both, first + need - 8))):
        assert refused(call(**bad)), bad
    assert b"overlaps" in L.mrs_tg_last_error(gpu_ctx._h)
    assert api.kernel_trace() == []
    torch.cuda.synchronize()
    assert bool(torch.all(fields == SENTINEL)) and bool(torch.all(ws == SENTINEL)) and not bool(both.any())
    # the whole-grid route needs no workspace, whatever is passed for it; a workspace that touches its neighbours is taken
    fields.copy_(gpu_ctx.field_from_occupancy(torch.zeros_like(occ), g, max_distance=1.0))
    assert call(max_distance=inf, workspace=None, workspace_bytes=0) == 0
    torch.cuda.synchronize()
    assert api.kernel_trace() == FULL_KERNELS + FULL_KERNELS
    api.kernel_trace_reset()
    fields.copy_(gpu_ctx.field_from_occupancy(torch.zeros_like(occ), g, max_distance=1.0))
    assert call(occupancy=at(both, first), workspace=at(both, first + voxels + (-voxels) % 8), field=ptr(fields)) == 0
    torch.cuda.synchronize()
    assert api.kernel_trace() == FULL_KERNELS + REGION_KERNELS
    # the Python layer: the tensors, the geometry, the scalars, the box, the workspace
    for kw in (dict(occupancy=occ.cpu()), dict(occupancy=occ.bool()), dict(occupancy=occ[:1]), dict(fields=fields.cpu()),
               dict(fields=fields.float()), dict(fields=fields[:1]), dict(fields=None), dict(geometry=None), dict(z_scale=0.0),
               dict(max_distance=nan), dict(field=2), dict(lo=(3, 2, 3)), dict(hi=(2, 2, 7)), dict(workspace=ws.cpu()),
               dict(workspace=ws.float()), dict(workspace=ws[:need // 8 - 1]), dict(workspace=fields.view(-1)),
               dict(workspace=ws.view(1, -1))):
        args = dict(occupancy=occ, fields=fields, geometry=g, lo=(2, 2, 3), hi=(2, 2, 3), field=1, max_distance=1.0, workspace=ws)
        args.update(kw)
        with pytest.raises(ValueError):
            gpu_ctx.field_update_region(**args)
    api.kernel_trace_reset()
    got = gpu_ctx.field_update_region(occ, fields, g, (2, 2, 3), (2, 2, 3), field=1, max_distance=1.0, workspace=ws)
    torch.cuda.synchronize()
    assert got is fields and api.kernel_trace() == REGION_KERNELS
    host = got.cpu().numpy()
    assert host[1, 3, 2, 2] == -0.25 and host[1, 3, 2, 3] == 0.25 and host[1, 3, 3, 2] == 0.5 and host[1, 0, 0, 0] == 1.0
    assert np.all(host[0] == 1.0)


def _seam_occupancy(geometry, seed):
    nx, ny, nz = geometry.dims
    return (np.random.default_rng(seed).random((1, nz, ny, nx)) < 0.02).astype(np.uint8)


def test_seam_field_clearance_on_the_updated_field(gpu_ctx):
    """three 4-segment paths, solve -> sample -> field_clearance: on the field updated on the device after a box in the paths'
    way changed and on the field rebuilt from the new occupancy, the same bits in clearance, cell, gradient and minimum -- and
    not what the old field gives"""
    batch, _, geometry, _ = fu.chain_batch()
    cap, dt, max_distance = fu.CHAIN_CAPACITY, fu.CHAIN_DT, 3.0
    old = _seam_occupancy(geometry, 11)
    times0 = gpu_ctx.solve_batch(batch, None)["times"]
    P = batch.n_paths
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        coeffs, _, status = autograd.solve(plan, dev(batch.fixed_mask), dev(batch.fixed_values), dev(times0))
        samples, n = autograd.sample(plan, coeffs, dev(times0), dt, cap, status)
        samples, n = samples.detach().contiguous(), n.contiguous()
        rows = np.minimum(n.cpu().numpy(), cap)
        assert P == 3 and np.all(rows > 0)
        # the box: three voxels a side around the middle row of the middle path, rerandomised at density 0.5
        at = samples.cpu().numpy()[1, rows[1] // 2, :3]
        node = np.rint((at - np.array(geometry.origin)) / np.array(geometry.spacing)).astype(int)
        last = np.array(geometry.dims) - 1
        lo, hi = tuple(int(x) for x in np.clip(node - 1, 0, last)), tuple(int(x) for x in np.clip(node + 1, 0, last))
        new = ru.changed_occupancy(old[0], lo, hi, 12)[None]
        assert not np.array_equal(old, new)
        info = api.field_update_query(geometry, lo, hi, max_distance=max_distance)
        assert info["reach"] == [6, 6, 6] and not info["whole_grid"]
        old_field = gpu_ctx.field_from_occupancy(dev(old), geometry, max_distance=max_distance)
        updated = old_field.clone()
        api.kernel_trace_reset()
        gpu_ctx.field_update_region(dev(new), updated, geometry, lo, hi, max_distance=max_distance)
        assert api.kernel_trace() == REGION_KERNELS
        rebuilt = gpu_ctx.field_from_occupancy(dev(new), geometry, max_distance=max_distance)
        torch.cuda.synchronize()
        c = dict(dims=geometry.dims, spacing=geometry.spacing, z_scale=1.0, max_distance=max_distance, signed=True, occupancy=new,
                 names=["seam"])
        assert eu.SAME_BITS(updated.cpu().numpy(), rebuilt.cpu().numpy()) and eu.SAME_BITS(updated.cpu().numpy(), eu.brute_force(c))
        results = []
        for field in (updated, rebuilt, old_field):
            o = dict(clearance=torch.empty((P, cap), dtype=torch.float64, device="cuda"),
                     cell=torch.empty((P, cap), dtype=torch.int32, device="cuda"),
                     gradient=torch.empty((P, cap, 4), dtype=torch.float64, device="cuda"),
                     min_clearance=torch.empty((P,), dtype=torch.float64, device="cuda"),
                     argmin=torch.empty((P, 2), dtype=torch.int32, device="cuda"))
            plan.field_clearance(samples, n, field, geometry, status=status, outside_value=max_distance, **o)
            torch.cuda.synchronize()
            results.append({k: v.cpu().numpy() for k, v in o.items()})
        a, b, before = results
        for k in ("clearance", "gradient", "min_clearance"):
            assert eu.SAME_BITS(a[k], b[k]), k
        assert np.array_equal(a["cell"], b["cell"]) and np.array_equal(a["argmin"], b["argmin"])
        # the comparison is about something: live rows whose clearance the change of the map moved
        live = a["cell"] >= 0
        assert np.array_equal(live, np.arange(cap)[None, :] < rows[:, None]) and np.all(np.isfinite(a["clearance"][live]))
        moved = live & (a["clearance"] != before["clearance"])
        assert moved.any() and moved[1].any()
    finally:
        plan.close()

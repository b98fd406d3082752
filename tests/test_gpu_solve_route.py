"""The route of the fixed-times solve, asked twice: of the library on the device (Plan.explain: the launchers run dry on the
route that route_solve gave them, and note their kernel) and of the same header on the CPU (tests/host/solve_route_harness.cpp,
with the device's compute-unit count), through the name mapping of tests/solve_route_util.py.  One case per instantiation a
launcher can choose, at the smallest shape that reaches it.  No kernel is launched.  The compute-unit count is read from the
device, so the two-sided kernel's bound is the device's own on a partitioned card; a case states its kernel by name where the
device is large enough for that name to hold (`min_cus`)."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from tests import solve_route_util as sr
from tests.solve_route_util import request

pytestmark = pytest.mark.gpu

MEL = dict(time_alloc_method=api.TIME_ALLOC_MELLINGER, estimate_times=1, sampling_dt=0.2, sample_capacity=512)
SNAP = dict(derivative_to_optimize=4)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return sr.build(tmp_path_factory.mktemp("solve_route_gpu"))


@pytest.fixture(scope="module")
def compute_units(gpu_ctx):
    import torch
    return torch.cuda.get_device_properties(gpu_ctx.device).multi_processor_count


@pytest.fixture(scope="module")
def lane_length(harness):
    """the shortest path the lane family takes: behind the last length of the tile kernel, found by the sweep"""
    got = sr.routes(harness, [request(1, S) for S in range(1, 257)])
    return 1 + [r["family"] for r in got].index("lane")


def _uniform(n, S):
    return (np.arange(n + 1, dtype=np.int64) * S).astype(np.int32)


def _bound(cus):
    return (5 * cus - 1) * 16 + 1   # the first size past the two-sided kernel's bound


# (id, paths (a number, or a function of the compute units), segments (a number or "lane"), options, group, harness request
#  keywords, the kernel by name, from how many compute units on that name holds)
CASES = [
    ("rows", 1, 3, SNAP, 0, {}, "solve_rows_kernel<0>", 1),
    ("rows_sampling", 1, 3, dict(sampling_dt=0.2, sample_capacity=512, **SNAP), 0, dict(sampling=1), "solve_rows_kernel<1>", 1),
    ("pipeline", 1, 3, dict(MEL, **SNAP), 0, "closing", ["solve_rows_pipeline_kernel"], 1),
    ("rows_tail", 1, 33, dict(MEL, **SNAP), 0, "closing", ["solve_rows_kernel<0>", "solve_rows_kernel<1>"], 1),
    ("tile_fused", 4, 200, SNAP, 0, {}, "solve_tile_kernel<true>", 1),
    ("tile_blocks", 1, 3, dict(flags=api.FLAG_MATERIALIZED_BLOCKS, **SNAP), 0, dict(fused=0), "solve_tile_kernel<false>", 1),
    ("lane", 1, "lane", SNAP, 0, {}, "(solve_linear_kernel<1, true>)", 1),
    ("duo", 6144, 2, SNAP, 0, {}, "solve_duo_kernel<false>", 77),
    ("duo_wp", 6144, 2, dict(flags=api.FLAG_POSITIONS_ARE_WAYPOINTS, **SNAP), 0, dict(wp=1), "solve_duo_kernel<true>", 77),
    ("quad_ends", 6144, 2, dict(derivative_to_optimize=2), 0, dict(d=2), "solve_quad_kernel<false, true>", 1),
    ("quad", _bound, 2, SNAP, 0, {}, "solve_quad_kernel<false>", 77),   # (fewer compute units: the bound lies below the four-lane size)
    ("rows_group", 1, 3, SNAP, 4, {}, "solve_rows_group_kernel", 1),
    ("duo_group_lean", 1024, 4, SNAP, 10, {}, "solve_duo_group_kernel<false, true>", 129),
    ("duo_group", 1023, 4, SNAP, 10, {}, "solve_duo_group_kernel<false>", 129),
    ("quad_group", 4096, 2, SNAP, 10, {}, "solve_quad_group_kernel<false>", 1),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_library_routes_as_the_header_says(gpu_ctx, harness, compute_units, lane_length, monkeypatch, case):
    name, n, S, options, group, kw, kernel, min_cus = case
    n = n(compute_units) if callable(n) else n
    S = lane_length if S == "lane" else S
    spell = name == "duo_group_lean"
    if spell:   # (read at every call)
        monkeypatch.setenv("MRS_TG_TRACE_INSTANTIATIONS", "1")
    plan = api.Plan(gpu_ctx, _uniform(n, S))
    try:
        told = plan.explain(api.default_options(**options), group_size=group)
    finally:
        plan.close()
    if kw == "closing":
        told = [k for k in told if k.startswith("solve_")]
        want = sr.closing_names(*sr.routes(harness, sr.closing_requests(n, S, cus=compute_units, d=options["derivative_to_optimize"])))
    else:
        if not options.get("flags", 0) & api.FLAG_MATERIALIZED_BLOCKS:
            assert len(told) == 1, told
        told = told[-1:]   # (materialised blocks: the kernel after the assembly)
        kernel = [kernel]
        want = [sr.kernel_name(sr.routes(harness, [request(n, S, group=group, cus=compute_units, **kw)])[0], spell)]
    assert told == want, (name, n, S, compute_units, told, want)
    if compute_units >= min_cus:
        assert told == kernel, (name, n, S, compute_units, told, kernel)

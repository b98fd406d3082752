"""The route of the Mellinger outer loop, asked twice: of the library on the device (Plan.explain: launch_nonlinear runs dry on the
route that route_nonlinear gave it, and notes its kernels) and of the same header on the CPU
(tests/host/nonlinear_route_harness.cpp, with the device's compute-unit count), through the name mapping of
tests/nonlinear_route_util.py.  One case per outer-loop kernel at the smallest shape that reaches it -- found by the CPU sweep,
not written down here -- and one queued launch.  No kernel is launched."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from tests import nonlinear_route_util as nr
from tests.nonlinear_route_util import request

pytestmark = pytest.mark.gpu

MEL = dict(time_alloc_method=api.TIME_ALLOC_MELLINGER, estimate_times=1, sampling_dt=0.2, sample_capacity=512)
LENGTHS = range(1, 129)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return nr.build(tmp_path_factory.mktemp("nonlinear_route_gpu"))


@pytest.fixture(scope="module")
def compute_units(gpu_ctx):
    import torch
    return torch.cuda.get_device_properties(gpu_ctx.device).multi_processor_count


@pytest.fixture(scope="module")
def sweep(harness, compute_units):
    """one path of every length under min-snap (4) and min-acceleration (2): the outer loop's kernels as the header names them"""
    return {d: [nr.outer_names(r) for r in nr.routes(harness, [request((1, S), d=d, cus=compute_units) for S in LENGTHS])] for d in (4, 2)}


# (id, objective order, the kernel that must lead the outer loop, the kernel behind it or None)
CASES = [
    ("wave", 4, "optimize_wave_kernel", None),
    ("split", 4, "optimize_split_kernel", None),
    ("lean_shared", 4, "optimize_lean_shared_kernel", "optimize_compact_kernel<false>"),
    ("lean_shared_ends", 2, "optimize_lean_shared_ends_kernel", "optimize_compact_kernel<true>"),
    ("lean_shared_ends_long", 4, "optimize_lean_shared_ends_long_kernel", "optimize_compact_kernel<false>"),
    ("lean", 4, "optimize_lean_kernel", "optimize_compact_kernel<false>"),
    ("lean_masked", 2, "optimize_lean_masked_kernel", "optimize_compact_kernel<true>"),
]


def _uniform(n, S):
    return (np.arange(n + 1, dtype=np.int64) * S).astype(np.int32)


def _explain(gpu_ctx, n, S, d):
    plan = api.Plan(gpu_ctx, _uniform(n, S))
    try:
        told = plan.explain(api.default_options(derivative_to_optimize=d, **MEL))
    finally:
        plan.close()
    return told[:-1] if told[-1] == "sample_kernel<NDER>" else told    # (the sampler is the plan's launch, not the outer loop's)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_library_routes_as_the_header_says(gpu_ctx, harness, compute_units, sweep, case):
    name, d, lead, behind = case
    want_outer = [lead] + ([behind] if behind else [])
    S = LENGTHS[sweep[d].index(want_outer)]      # the smallest shape that reaches the kernel
    told = _explain(gpu_ctx, 1, S, d)
    want = nr.kernel_names(nr.routes(harness, [request((1, S), d=d, cus=compute_units)])[0])
    assert told == want and told[:len(want_outer)] == want_outer, (name, S, compute_units, told, want)


def test_a_launch_larger_than_the_device_holds_is_queued(gpu_ctx, harness, compute_units):
    resident = compute_units * 4 * 2         # two wavefronts per SIMD; four paths of 10 segments per wavefront
    for n, queued in ((4 * resident, False), (4 * resident + 1, True)):
        r = nr.routes(harness, [request((n, 10), cus=compute_units, resident=resident)])[0]
        told = _explain(gpu_ctx, n, 10, 4)
        assert told == nr.kernel_names(r) and (told[0] == "set_queue_kernel") == bool(r["queued"]), (n, compute_units, told, r)
        if n > 2560:     # (a device of fewer than 80 compute units: so few paths split the dimensions and run no lean kernel)
            assert bool(r["queued"]) == queued, (n, compute_units, r)

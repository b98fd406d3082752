"""policy_steps.optimize_paths with the two options it used to refuse: override_heading_atan2 (Plan.travel_heading over the
finished samples, in place) behind the optimiser's rounds, against api.optimize_paths under the same policy on the 24 requests of
tests/test_gpu_pathedit_loop.py; and fallback_sampling with override_heading_atan2 (findTrajectoryFallback composed from plan
steps) against the CPU oracle on the ten paths and the stop_at pattern of
tests/test_gpu_policy.py::test_fallback_sampler_and_atan2_heading_match_oracle, by that test's criteria."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api, policy_steps
from mrs_uav_trajectory_generation_amd import problem as pr
from oracle import pyoracle as po
from tests import heading_util as hu

pytestmark = pytest.mark.gpu


def test_optimiser_route_with_the_heading_override_matches_the_host_loop(gpu_ctx):
    """The two loops run the same kernels on the same waypoints: success, the counts and the positions are held to equality, and
    the headings of the rows 0 .. n-2 -- device atan2 here, the host's in mrs_tg_optimize_paths, on the same bits -- to the
    measured bound, directly and not cyclically."""
    paths = [pr.random_walk_waypoints(4 + (i % 5), 500 + i) for i in range(24)]
    pol = api.default_policy_options(solver=dict(derivative_to_optimize=4), override_heading_atan2=1)
    out = policy_steps.optimize_paths(gpu_ctx, paths, policy=pol, sample_capacity=2048)
    ref = api.optimize_paths(gpu_ctx, paths, policy=pol, sample_capacity=2048)
    plain = policy_steps.optimize_paths(gpu_ctx, paths, policy=api.default_policy_options(solver=dict(derivative_to_optimize=4)),
                                        sample_capacity=2048)
    samples, kept = out["samples"].cpu().numpy(), plain["samples"].cpu().numpy()
    for k in ("success", "n_samples", "n_waypoints", "iterations"):
        assert np.array_equal(out[k], ref[k]), (k, out[k], ref[k])
    worst, rows = 0.0, 0
    for p in range(len(paths)):
        n = int(out["n_samples"][p])
        assert hu.same_bits(samples[p, :n, :3], ref["samples"][p, :n, :3]), p
        assert hu.same_bits(samples[p, :, :3], kept[p, :, :3]), p             # the override touches headings only
        if n:
            assert hu.same_bits(samples[p, n - 1:, 3], kept[p, n - 1:, 3]), p   # the last row keeps its sampled yaw
        if n > 1:
            worst = max(worst, float(np.max(np.abs(samples[p, :n - 1, 3] - ref["samples"][p, :n - 1, 3]))))
            rows += n - 1
    print("POLICY STEPS HEADING: %d successes, %d rows, worst |heading - host loop's| %.3e (bound %.3e)" %
          (int(out["success"].sum()), rows, worst, hu.HEADING_BOUND))
    assert out["success"].sum() >= 20 and rows > 500
    assert worst <= hu.HEADING_BOUND


def test_fallback_route_with_the_heading_override_matches_the_oracle(gpu_ctx):
    paths = [pr.random_box_waypoints(4 + (i % 5), 40 + i) for i in range(10)]
    stops = [[(i == 2) for i in range(len(p))] for p in paths]
    pol = api.default_policy_options(fallback_sampling=1, override_heading_atan2=1)
    out = policy_steps.optimize_paths(gpu_ctx, paths, stop_flags=stops, policy=pol, sample_capacity=4096)
    samples = out["samples"].cpu().numpy()
    for p, wp in enumerate(paths):
        ref = po.optimize_path(wp, stop_at=stops[p], limits=pr.DEFAULT_LIMITS,
                               policy=po.default_policy(fallback_sampling=1, override_heading_atan2=1), capacity=4096)
        assert out["success"][p] == ref["success"] == 1
        n = ref["n_samples"]
        assert out["n_samples"][p] == n
        assert np.max(np.abs(samples[p, :n, :3] - ref["samples"][:, :3])) < 1e-12
        dh = np.abs(samples[p, :n, 3] - ref["samples"][:, 3])
        assert np.max(np.minimum(dh, 2 * np.pi - dh)) < 1e-9

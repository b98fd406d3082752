"""policy_steps.optimize_paths -- the reference's optimize() composed from plan steps, the waypoints on the device throughout
(thinning, unwrap, vertices, Baca total, solve with samples, both gates, deviation, subdivision, next plan) -- on the 24 requests
of tests/test_gpu_policy.py::test_policy_loop_matches_oracle, against the CPU oracle's optimize_path under that test's criteria.
On the oracle all 24 give the same success, counts and iterations at max_deviation 0.05 - 1e-4, 0.05 and 0.05 + 1e-4: no
decision sits near the threshold; 22 insert mid-points, over up to 4 rounds; request 20 fails on every run."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api, policy_steps
from mrs_uav_trajectory_generation_amd import problem as pr
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def test_device_resident_loop_matches_oracle(gpu_ctx):
    paths = [pr.random_walk_waypoints(4 + (i % 5), 500 + i) for i in range(24)]
    pol = api.default_policy_options(solver=dict(derivative_to_optimize=4))
    out = policy_steps.optimize_paths(gpu_ctx, paths, policy=pol, sample_capacity=2048)
    samples = out["samples"].cpu().numpy()
    same = subdivided = 0
    for p, wp in enumerate(paths):
        ref = po.optimize_path(wp, limits=pr.DEFAULT_LIMITS, deriv=4, capacity=2048)
        assert out["success"][p] == ref["success"], p
        subdivided += int(ref["iterations"] > 0)
        print("path %d: success %d / %d, waypoints %d / %d, iterations %d / %d, samples %d / %d" % (
            p, out["success"][p], ref["success"], out["n_waypoints"][p], ref["n_waypoints"], out["iterations"][p],
            ref["iterations"], out["n_samples"][p], ref["n_samples"]))
        if (out["n_waypoints"][p] == ref["n_waypoints"] and out["iterations"][p] == ref["iterations"]
                and out["n_samples"][p] == ref["n_samples"]):
            n = ref["n_samples"]
            if n == 0 or np.max(np.abs(samples[p, :n, :3] - ref["samples"][:, :3])) < 1e-6:
                same += 1
    print("RATE policy_steps: %d / %d" % (same, len(paths)))
    assert subdivided >= 20        # the loop is exercised: most requests insert mid-points
    assert same >= len(paths) - 1, same

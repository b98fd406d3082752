"""Paths stamped in the future and requests before takeoff, on the GPU.

* Python: 64 random requests, each with a smooth synthetic 41-sample MPC prediction, through api.prepare_initial_condition ->
  api.optimize_paths (0.2 s sampling for the paths from the future) -> api.splice_prediction
  (the reference's src/mrs_trajectory_generation.cpp:506-674, 692-697, 801-838).
* C++: examples/future_path_host.cpp, include/mrs_tg_service.hpp on a fixed clock, built with g++ against libmrs_tg.so; its
  responses checked the way the reference's get_path tests check the nodelet's (test/include/get_path_test.h) and bit for bit
  against the same solve issued through api.optimize_paths."""
import json
import os
import subprocess

import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from mrs_uav_trajectory_generation_amd.problem import DEFAULT_LIMITS
from tests.test_gpu_reference_scenarios import TEST_PATH, check_trajectory, check_waypoint_idxs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PRED = 41
CAPACITY = 8192   # ServiceParams::sample_capacity


def ref_k(offset):
    return int(np.ceil((offset * 0.50 - 0.01) / 0.2)) + 1


def ref_k2(age):
    return int(np.floor((age - 0.01) / 0.2)) + 1


def sample_times():
    return np.array([0.0] + [0.01 + 0.2 * (i - 1) for i in range(1, N_PRED)])


def synthetic_prediction(rng):
    """a UAV cruising along a bearing with a slowly changing speed and heading: derivatives agree with the positions"""
    t = sample_times()
    theta, h0 = rng.uniform(-np.pi, np.pi, 2)
    d = np.array([np.cos(theta), np.sin(theta), 0.0])
    s, a = rng.uniform(0.5, 1.2), rng.uniform(-0.05, 0.05)
    w = rng.uniform(-0.1, 0.1)
    p0 = np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(2.5, 4.0)])
    pos = np.zeros((N_PRED, 4))
    vel = np.zeros((N_PRED, 4))
    acc = np.zeros((N_PRED, 4))
    pos[:, :3] = p0 + np.outer(s * t + 0.5 * a * t * t, d)
    pos[:, 3] = h0 + w * t
    vel[:, :3] = np.outer(s + a * t, d)
    vel[:, 3] = w
    acc[:, :3] = a * d
    pred = dict(position=pos, velocity=vel, acceleration=acc, jerk=np.zeros((N_PRED, 4)))
    return pred, (p0, d, s, a, h0, w, theta)


def planner_path(rng, motion, offset, n_seg):
    """the path a planner sends: its first waypoint where the UAV will be at the stamp, then onwards in 2-4 m steps"""
    p0, d, s, a, h0, w, theta = motion
    first = np.concatenate([p0 + (s * offset + 0.5 * a * offset * offset) * d, [h0 + w * offset]])
    pts = [first]
    bearing, cur = theta, first[:3].copy()
    hdg = first[3]
    for i in range(n_seg):
        bearing += rng.uniform(-0.3, 0.3) if i > 0 else 0.0    # on along the prediction's course first
        cur = cur + rng.uniform(2.0, 4.0) * np.array([np.cos(bearing), np.sin(bearing), 0.0])
        cur[2] = np.clip(cur[2] + rng.uniform(-0.3, 0.3), 2.0, 5.0)
        hdg += rng.uniform(-0.2, 0.2)
        pts.append(np.concatenate([cur, [hdg]]))
    return np.array(pts)


def _close(sample, row, tol=1e-9):
    """equal to tol, the heading modulo 2 pi (the sampler returns it wrapped into (-pi, pi])"""
    d = np.asarray(sample, dtype=np.float64) - np.asarray(row, dtype=np.float64)
    d[3] = (d[3] + np.pi) % (2.0 * np.pi) - np.pi
    return np.max(np.abs(d)) < tol


def _policy(dt, **overrides):
    return api.default_policy_options(solver=dict(time_alloc_method=api.TIME_ALLOC_MELLINGER, derivative_to_optimize=2,
                                                  sampling_dt=dt), **overrides)


@pytest.mark.parametrize("seed,max_deviation", [(3, None), (20261015, 0.25)])
def test_prepare_optimize_splice_pipeline(gpu_ctx, seed, max_deviation):
    """Seed 3 under the reference's default policy (deviation bound 0.05 m): the CPU oracle of the policy loop
    (oracle/mto_policy.c) accepts every one of its 64 requests.  Seed 20261015 with a 0.25 m bound, as a planner may send in
    max_deviation_from_path: under 0.05 m the deviation check gives up on one of its random turns, in the oracle as well."""
    rng = np.random.default_rng(seed)
    offsets = rng.uniform(0.0, 5.0, 64)
    offsets[:4] = [0.05, 0.2, np.nextafter(0.2, 1.0), 5.0]
    reqs = []
    for r in range(64):
        pred, motion = synthetic_prediction(rng)
        wps = planner_path(rng, motion, offsets[r], int(rng.integers(6, 11)))
        tracker = dict(position=pred["position"][0], velocity=pred["velocity"][0], acceleration=pred["acceleration"][0],
                       jerk=pred["jerk"][0])
        dec = api.prepare_initial_condition(tracker, 0.1, pred, None, 0.0, float(offsets[r]), len(wps), False)
        assert dec["has_initial_condition"]
        assert dec["from_future"] == (offsets[r] > 0.2)           # 5 s ahead is k = 14, well inside 41 samples
        assert dec["drop_first_waypoint"] == (offsets[r] > 0.2)
        path = np.vstack([dec["waypoint"], wps[1:] if dec["drop_first_waypoint"] else wps])
        reqs.append(dict(pred=pred, dec=dec, path=path))
    for future, dt in ((True, 0.2), (False, 0.1)):
        idx = [i for i, q in enumerate(reqs) if q["dec"]["from_future"] == future]
        assert idx
        out = api.optimize_paths(gpu_ctx, [reqs[i]["path"] for i in idx], initial_states=[reqs[i]["dec"]["initial_state"] for i in idx],
                                 policy=_policy(dt) if max_deviation is None else _policy(dt, max_deviation=max_deviation),
                                 sample_capacity=2048)
        assert np.all(out["success"] == 1), out["success"]
        for j, i in enumerate(idx):
            q = reqs[i]
            samples = out["samples"][j, :out["n_samples"][j]]
            assert _close(samples[0], q["dec"]["waypoint"])
            if not future:
                continue
            k = q["dec"]["sample_offset"]
            assert k == ref_k(offsets[i])
            spliced = api.splice_prediction(q["pred"], k, 0.05, samples)       # 0.05 s old: k2 = 1 < k
            assert spliced.shape[0] == samples.shape[0] + k
            assert spliced[k:].tobytes() == samples.tobytes()
            assert spliced[:k].tobytes() == q["pred"]["position"][:k].tobytes()
            assert _close(spliced[k], q["pred"]["position"][k])


# ---- the service layer: examples/future_path_host.cpp ----

STRAIGHT = np.array([[2, 0, 3, 0], [6, 0, 3, 0], [10, 0, 3, 0], [10, 4, 3, 0]], dtype=np.float64)
TRACKER = np.array([0.0, 0.0, 3.0, 0.0])


def host_prediction():
    t = sample_times()
    pos = np.zeros((N_PRED, 4))
    pos[:, 0] = t
    pos[:, 2] = 3.0
    return pos


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("future_host") / "future_path_host")
    libdir = os.path.join(ROOT, "mrs_uav_trajectory_generation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "future_path_host.cpp"), "-o", exe, "-L", libdir, "-lmrs_tg",
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout
    res = json.loads(out)
    for v in res.values():
        if isinstance(v, dict):
            v["points"] = np.array(v["points"], dtype=np.float64).reshape(-1, 4)
    return res


def _solve_alone(ctx, path, init, dt, stop_flags=None, limits=DEFAULT_LIMITS):
    out = api.optimize_paths(ctx, [path], initial_states=[init], stop_flags=stop_flags, limits=np.asarray(limits)[None, :],
                             policy=_policy(dt), sample_capacity=CAPACITY)
    assert out["success"][0] == 1
    return out["samples"][0, :out["n_samples"][0]]


def _state(heading=0.0, velocity=(0, 0, 0, 0)):
    return dict(heading=heading, velocity=list(velocity), acceleration=[0, 0, 0, 0], jerk=[0, 0, 0, 0])


def test_before_takeoff_starts_at_the_takeoff_height(host_output):
    r = host_output["before_takeoff"]
    assert r["success"] and r["message"] == "trajectory generated" and r["dt"] == 0.2 and r["fly_now"]
    pts = r["points"]
    assert np.max(np.abs(pts[0] - [0.0, 0.0, 1.5, 0.5])) < 1e-9
    assert check_trajectory(pts, TEST_PATH) and check_waypoint_idxs(r["idxs"], TEST_PATH)


def test_path_stamped_two_seconds_ahead(host_output, gpu_ctx):
    r = host_output["future"]
    assert r["success"] and r["dt"] == 0.2            # although sampling_dt is 0.1
    k = ref_k(2.0)
    assert k == 6 and ref_k2(0.05) < k
    pred = host_prediction()
    pts = r["points"]
    assert pts[:k].tobytes() == pred[:k].tobytes()    # the prefix: prediction rows 0 .. k-1
    assert np.max(np.abs(pts[k] - pred[k])) < 1e-9
    # the first waypoint is dropped: the solved part is the solve of [row k, waypoints 1..] at 0.2 s, bit for bit
    solved = _solve_alone(gpu_ctx, np.vstack([pred[k], STRAIGHT[1:]]), _state(0.0, (1, 0, 0, 0)), 0.2)
    assert pts[k:].tobytes() == solved.tobytes()
    # the indices over the path as requested, the dropped waypoint included (:2392)
    assert check_waypoint_idxs(r["idxs"], STRAIGHT) and check_trajectory(pts, STRAIGHT)
    assert r["idxs"] == api.waypoint_trajectory_idxs(pts, STRAIGHT).tolist()


def test_stamp_beyond_the_horizon_starts_at_the_tracker_command(host_output, gpu_ctx):
    r = host_output["beyond_horizon"]
    assert r["success"] and r["dt"] == 0.1
    pts = r["points"]
    assert np.max(np.abs(pts[0] - TRACKER)) < 1e-9
    solved = _solve_alone(gpu_ctx, np.vstack([TRACKER, STRAIGHT[1:]]), _state(0.0, (1, 0, 0, 0)), 0.1)
    assert pts.tobytes() == solved.tobytes()          # no prefix, and the first waypoint dropped
    assert np.min(np.linalg.norm(pts[:, :3] - [-3, 5, 3], axis=1)) > 1.0


def test_present_request_and_mixed_batch(host_output, gpu_ctx):
    r = host_output["present"]
    assert r["success"] and r["dt"] == 0.1
    solved = _solve_alone(gpu_ctx, np.vstack([TRACKER, STRAIGHT]), _state(0.0, (1, 0, 0, 0)), 0.1)
    assert r["points"].tobytes() == solved.tobytes()
    assert host_output["mixed_equals_alone"] is True


def test_stale_tracker_command_uses_the_uav_state(host_output):
    for name in ("stale_tracker", "stale_tracker_future"):
        r = host_output[name]
        assert r["success"] and r["dt"] == 0.1, name
        assert np.max(np.abs(r["points"][0] - [0.0, 0.0, 4.5, 0.0])) < 1e-9, name
    assert check_trajectory(host_output["stale_tracker"]["points"], TEST_PATH)


def test_without_the_new_inputs_the_service_answers_as_before(host_output, gpu_ctx):
    """the service before stamps existed: the current state prepended, sampling_dt, the limits of findTrajectory (:985-1037,
    a user override that the state at rest allows), the reference's error string, the indices over the requested waypoints"""
    cur = np.array([0.0, 0.0, 3.0, 0.5])
    # {v, a, j} x {horizontal, vertical, heading}: the override's 4 / 2, 3 / 2, 30 / 30 and the constraints' heading limits
    override = [4.0, 2.0, 1.0, 3.0, 2.0, 2.0, 30.0, 30.0, 20.0]
    for name, wps, stop, limits in (("untouched_plain", TEST_PATH, None, DEFAULT_LIMITS),
                                    ("untouched_loop", np.vstack([TEST_PATH, TEST_PATH[:1]]), [0, 1, 1, 1, 1, 1], DEFAULT_LIMITS),
                                    ("untouched_override", TEST_PATH, None, override)):
        r = host_output[name]
        assert r["success"] and r["message"] == "trajectory generated" and r["dt"] == 0.2 and r["fly_now"], name
        solved = _solve_alone(gpu_ctx, np.vstack([cur, wps]), _state(0.5), 0.2, stop_flags=None if stop is None else [stop],
                              limits=limits)
        assert r["points"].tobytes() == solved.tobytes(), name
        assert r["idxs"] == api.waypoint_trajectory_idxs(solved, wps).tolist(), name
        assert check_waypoint_idxs(r["idxs"], wps)
    assert len(host_output["untouched_override"]["points"]) < len(host_output["untouched_plain"]["points"])
    e = host_output["untouched_empty"]
    assert (e["success"], e["message"], len(e["points"])) == (False, "received an empty message", 0)
    # a tracker stamp, a prediction and a UAV state that do not apply to unstamped paths change no bit of any answer
    assert host_output["inputs_that_do_not_apply_change_nothing"] is True

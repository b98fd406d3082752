"""The transfer routes of the one-call host interface (mrs_tg_solve_batch / solve_batch_samples_only, DESIGN.md "Transfer
routes of the one-call interface"): wherever the caller keeps an array -- pinned, pageable and small (staged), pageable and
large, registered in place -- and whatever MRS_TG_STAGE_MAX_BYTES and MRS_TG_ZERO_COPY say, every output array holds the same
bits, and api.kernel_trace() tells which route a call took.

tests/golden/host_call_routes.json came from the PARENT of the commit that split the interface into a transfer plan
(aab13a9, "Share batch addressing and path-wavefront helpers; name the variants"): this file's generator,

    python -m tests.test_gpu_host_call_routes --generate tests/golden/host_call_routes.json

run on an MI355X with that commit's library.  It records, for every setting, case and route, the kernel names of the call and
the SHA-256 of every output array; the library under test has to reproduce both.  The fixture is data of the parent commit:
it is not regenerated from the code under test.  (Its lists name sample_acc_table_kernel where the generator's process happened
to sample for the first time; ONCE_PER_PROCESS below is left out of every comparison.)

The knobs are read once per process, so each setting runs in a fresh child process (started, never exec'ed into).

Case (e) is not the fixed-times batch of five six-segment paths one might expect beside (a) - (d): solve_batch_samples_only has
one public caller, mrs_tg_optimize_paths, which chooses the times itself (Mellinger) and keeps the arrays of a round in its own
block.  So (e) is five requests of six segments through that caller, and the routes of its block are settings of the process:
pinned by default, staged and large pageable under MRS_TG_POLICY_PINNED=0 (SETTINGS)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api, problem as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "host_call_routes.json")
PARENT_COMMIT = "aab13a9"

ROUTES = ("pageable", "pinned", "pinned_values", "registered_coeffs")
SETTINGS = {
    "stage_max_0": {"MRS_TG_STAGE_MAX_BYTES": "0"},
    "zero_copy_0": {"MRS_TG_ZERO_COPY": "0"},
    # case (e) keeps its arrays in the context's pinned scratch; with the scratch in ordinary memory the samples-only call (no
    # coefficients destination, no cost) has its arrays staged, and with nothing staged they travel as large pageable arrays
    "policy_pageable": {"MRS_TG_POLICY_PINNED": "0"},
    "policy_pageable_unstaged": {"MRS_TG_POLICY_PINNED": "0", "MRS_TG_STAGE_MAX_BYTES": "0"},
}
OUTPUTS = ("times", "coeffs", "status", "cost", "n_samples", "samples")


def _fixed_times(batch):
    return 1.0 + 0.25 * (np.arange(batch.n_segments) % 5)


def _cases():
    """name -> (batch, seg_times or None, options): the smallest shapes that reach each branch of the interface"""
    mixed = pr.random_mixed_batch(6, seed0=11)
    moving = pr.random_batch(4, 14, seed0=3)       # 13 .. 15 segments: the window of the moving-start hint
    v0 = int(moving.seg_offsets[2]) + 2            # first vertex of path 2: its velocity slot is constrained (a path's end)
    assert moving.fixed_mask[v0, 1] == 1
    moving.fixed_values[v0, 1] = (0.5, -0.3, 0.2, 0.0)
    short = pr.random_batch(3, 2, seed0=7)
    return {
        "a_fixed_times": (mixed, _fixed_times(mixed), {}),
        "b_fixed_times_sampled": (mixed, _fixed_times(mixed), dict(sampling_dt=0.2, sample_capacity=64)),
        "c_mellinger_moving_start": (moving, None, dict(time_alloc_method=api.TIME_ALLOC_MELLINGER, sampling_dt=0.2,
                                                        sample_capacity=256)),
        "d_estimate_times": (short, None, {}),
    }


def _canonical(out, capacity):
    """the output arrays of a call, copied; sample rows beyond min(n_samples, capacity) are nobody's (a pinned sample array
    receives the produced rows only) and read as zero here"""
    res = {k: np.array(out[k]) for k in OUTPUTS if out.get(k) is not None}
    if "samples" in res:
        for p, n in enumerate(np.minimum(res["n_samples"], capacity)):
            res["samples"][p, n:] = 0
    return res


# launched by the first sampling call of a process, whichever call that is (the sampler's tables live until the last context
# goes): part of a process's history, not of a call's route
ONCE_PER_PROCESS = ("sample_acc_table_kernel",)


def _route_kernels(trace):
    return [k for k in trace if k not in ONCE_PER_PROCESS]


def _traced(call):
    api.kernel_trace_reset()
    out = call()
    return out, _route_kernels(api.kernel_trace())


def _solve_by_route(ctx, route, batch, times, kw):
    """one case through one route -> (canonical outputs, kernel names of the route's last call)"""
    L = api.load_library()
    cap = kw.get("sample_capacity", 0)
    if route == "pageable":
        out, trace = _traced(lambda: ctx.solve_batch(batch, times, **kw))
        return _canonical(out, cap), trace
    pinned = pr.Batch(batch.seg_offsets, api.pinned_copy(batch.waypoints), api.pinned_copy(batch.fixed_mask),
                      api.pinned_copy(batch.fixed_values), api.pinned_copy(batch.limits), batch.derivative_to_optimize)
    if route == "pinned":   # every array pinned, the same arrays for two calls: the second re-uses arenas and plan
        P, nS = batch.n_paths, batch.n_segments
        out = dict(times=api.pinned_empty(nS), coeffs=api.pinned_empty((nS, 4, 10)), status=api.pinned_empty(P, np.int32),
                   cost=api.pinned_empty(P), n_samples=api.pinned_empty(P, np.int32), samples=api.pinned_empty((P, max(cap, 1), 4)))
        results = []
        for _ in range(2):
            for a in out.values():
                a[...] = 0
            got, trace = _traced(lambda: ctx.solve_batch(pinned, times, out=out, **kw))
            results.append(_canonical(got, cap))
        for k in results[0]:
            assert np.array_equal(results[0][k], results[1][k]), ("pinned, first and second call", k)
        return results[1], trace
    mixed = pr.Batch(batch.seg_offsets, batch.waypoints, batch.fixed_mask, pinned.fixed_values, batch.limits,
                     batch.derivative_to_optimize)
    if route == "pinned_values":
        out, trace = _traced(lambda: ctx.solve_batch(mixed, times, **kw))
        return _canonical(out, cap), trace
    assert route == "registered_coeffs"   # a pageable coefficient array pinned in place by registration
    keep = ctx.solve_batch(mixed, times, **kw)
    assert L.mrs_tg_host_register(keep["coeffs"].ctypes.data, keep["coeffs"].nbytes) == 0
    try:
        keep["coeffs"][...] = 0
        out, trace = _traced(lambda: ctx.solve_batch(mixed, times, out=keep, **kw))
        res = _canonical(out, cap)
    finally:
        assert L.mrs_tg_host_unregister(keep["coeffs"].ctypes.data) == 0
    return res, trace


def _policy_case(ctx):
    """case (e): five requests of six segments through mrs_tg_optimize_paths -- below the 64 requests from which a round runs
    on the device, so every round is one solve_batch_samples_only (no coefficients destination, no cost); see the module's
    docstring for how it differs from the other cases"""
    paths = [pr.random_box_waypoints(6, p) for p in range(5)]
    cap = 1024
    out, trace = _traced(lambda: api.optimize_paths(ctx, paths, sample_capacity=cap))
    res = {k: np.array(v) for k, v in out.items()}
    for p, n in enumerate(np.minimum(res["n_samples"], cap)):
        res["samples"][p, n:] = 0
    return res, trace


def run_all(ctx):
    """{case: {route: (outputs, trace)}} of this process, under whatever knobs its environment sets"""
    results = {}
    for name, (batch, times, kw) in _cases().items():
        results[name] = {route: _solve_by_route(ctx, route, batch, times, kw) for route in ROUTES}
    results["e_samples_only"] = {"policy": _policy_case(ctx)}
    return results


def _flat(results):
    """-> ({"case/route/array": array}, {"case/route": [kernel names]})"""
    arrays, traces = {}, {}
    for case, routes in results.items():
        for route, (out, trace) in routes.items():
            traces[case + "/" + route] = trace
            for k, a in out.items():
                arrays["%s/%s/%s" % (case, route, k)] = a
    return arrays, traces


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def _child(setting, path):
    """a fresh process with the setting's knobs: runs every case and leaves its arrays and traces at `path`"""
    env = dict(os.environ, **SETTINGS[setting])
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_host_call_routes", "--child", path], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (setting, p.stdout[-2000:], p.stderr[-4000:])
    with np.load(path) as z:
        traces = json.loads(str(z["__traces__"]))
        return {k: z[k] for k in z.files if k != "__traces__"}, traces


@pytest.fixture(scope="module")
def own(gpu_ctx):
    return _flat(run_all(gpu_ctx))


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_call_routes")
    return {setting: _child(setting, str(d / (setting + ".npz"))) for setting in SETTINGS}


@pytest.fixture(scope="module")
def fixture_of_parent():
    with open(FIXTURE) as f:
        data = json.load(f)
    assert data["commit"] == PARENT_COMMIT
    return data["settings"]


def test_every_route_gives_the_bits_of_the_all_pageable_call(own):
    arrays, _ = own
    compared = 0
    for key, a in arrays.items():
        case, route, k = key.split("/")
        if route in ("pageable", "policy"):
            continue
        assert np.array_equal(a, arrays["%s/pageable/%s" % (case, k)]), key
        compared += 1
    assert compared == 3 * (4 + 6 + 6 + 4)   # routes x output arrays of cases a (no sampling), b, c, d (no sampling)


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_every_setting_of_the_knobs_gives_the_same_bits(own, children, setting):
    arrays, _ = own
    got, _ = children[setting]
    assert sorted(got) == sorted(arrays)
    for key in arrays:
        assert np.array_equal(got[key], arrays[key]), (setting, key)


def test_the_kernel_trace_tells_zero_copy_from_the_copying_routes(own, children):
    def copies(traces, route):
        return sum(k.startswith("copy_many_kernel") for k in traces["a_fixed_times/" + route])
    assert copies(own[1], "pinned") == 0                        # zero copy: the solve reads and writes the caller's arrays
    assert copies(children["zero_copy_0"][1], "pinned") == 2    # one gather, one scatter
    assert copies(own[1], "pageable") == 2                      # the staged span up, the staged span down


def test_kernels_and_bits_are_those_of_the_parent_commit(own, children, fixture_of_parent):
    runs = dict(children, default=own)
    assert sorted(fixture_of_parent) == sorted(runs)
    for setting, (arrays, traces) in runs.items():
        want = fixture_of_parent[setting]
        assert traces == {k: _route_kernels(t) for k, t in want["traces"].items()}, setting
        assert {k: _sha(a) for k, a in arrays.items()} == want["sha256"], setting


def _main(argv):
    ctx = api.Context(0)
    if argv[0] == "--child":
        arrays, traces = _flat(run_all(ctx))
        np.savez(argv[1], __traces__=np.array(json.dumps(traces)), **arrays)
    elif argv[0] == "--generate":   # on the commit whose behaviour is to be recorded
        settings = {}
        arrays, traces = _flat(run_all(ctx))
        settings["default"] = dict(traces=traces, sha256={k: _sha(a) for k, a in arrays.items()})
        for setting in SETTINGS:
            arrays, traces = _child(setting, argv[1] + "." + setting + ".npz")
            os.remove(argv[1] + "." + setting + ".npz")
            settings[setting] = dict(traces=traces, sha256={k: _sha(a) for k, a in arrays.items()})
        with open(argv[1], "w") as f:
            json.dump(dict(commit=PARENT_COMMIT, settings=settings), f, indent=1, sort_keys=True)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    _main(sys.argv[1:])

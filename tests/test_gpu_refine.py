"""MRS_TG_FLAG_REFINE on the GPU (refine_kernel, mrs_tg_refine.hip): the refinement pass behind the final solve of every mode.

Every accuracy assertion is against the oracle's 113-bit route (the reference's algorithm without its rounding) or the
60-digit fixtures of tests/golden (linear_qp_cases.json, refine_cases.json):

  * bench.py's twenty slots (the headline test's recipe, each slot solved with Plan.solve and the flag): every one of the
    20 480 paths within 1e-11 -- without the flag three are above 1e-8, the worst 4.8e-8 -- and the cost to 1e-12;
  * every fixture but the guard case within 1e-11 of its 60-digit coefficients; the guard case (a 1e-4 s segment between 10 s
    ones, where corrections solved in double stop lowering the residual) keeps its status and times and is no worse than
    without the flag;
  * Mellinger and mode 0 on 1024 x 10, Mellinger on the 8192-path ragged batch: times and status the bits of the same call
    without the flag (and without sampling), coefficients at the returned times within 1e-11 of the 113-bit route;
  * the same with every pool block poisoned (MRS_TG_POOL_POISON=1, a child process): the refinement reads no workspace
    element it did not write -- the paths whose last vertex has free slots included;
  * samples taken from the refined coefficients; find_trajectory / optimize_paths (host and device rounds) run the kernel and
    decide as without it; identical calls give identical bits; plan_explain; the grouped launch refuses the flag.
"""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import api, problem as pr
from oracle import pyoracle as po
from tests import util

pytestmark = pytest.mark.gpu

SLOTS, PATHS, SEGMENTS = 20, 1024, 10
TOL_REFINED = 1e-11
GUARD_CASE = "guard_1em4_between_10s"
# neighbour-time ratio beyond which a correction solved in double cannot converge ((T_max / T_min)^(2d - 1) * eps > 1): there
# the guard keeps the solve's answer, which is asserted to be no worse instead
GUARD_REGIME_COND = 1e15


def _per_path_error(so, got, ref):
    return np.array([util.coeff_error(got[a:b], ref[a:b]) for a, b in zip(so[:-1], so[1:])])


def _neighbour_cond(so, t, d):
    out = []
    for a, b in zip(so[:-1], so[1:]):
        tt = t[a:b]
        r = max([max(tt[i], tt[i + 1]) / min(tt[i], tt[i + 1]) for i in range(len(tt) - 1)] or [1.0])
        out.append(r ** (2 * d - 1))
    return np.array(out)


def _quad(batch, t, d):
    with po.arithmetic(po.QUAD_PRECISION):
        return po.solve_batch(batch.seg_offsets, batch.waypoints, batch.fixed_mask, batch.fixed_values, batch.limits, t, deriv=d,
                              n_threads=16)


def test_the_library_reports_the_capability():
    assert api.capabilities() & api.CAP_REFINE
    assert api.FLAG_REFINE == 256


def test_bench_slots_every_path_within_1e_11_of_the_113_bit_route(gpu_ctx):
    so = pr.random_batch(PATHS, SEGMENTS, seed0=0).seg_offsets
    plan = api.Plan(gpu_ctx, so)
    est = api.default_options(derivative_to_optimize=4, estimate_times=1)
    ref = api.default_options(derivative_to_optimize=4, flags=api.FLAG_REFINE)
    worst, above, errs = 0.0, [], []
    try:
        for s in range(SLOTS):
            batch = pr.random_batch(PATHS, SEGMENTS, seed0=s * PATHS)
            db = api.DeviceBatch(batch, "cuda:0")
            plan.solve(est, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost, waypoints=db.waypoints,
                       limits=db.limits)
            db.coeffs.zero_()
            db.cost.zero_()
            db.status.zero_()
            api.kernel_trace_reset()
            plan.solve(ref, db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs, db.status, db.cost)
            trace = api.kernel_trace()
            torch.cuda.synchronize()
            assert trace[-1] == "refine_kernel", trace
            t, c, st, cost = db.seg_times.cpu().numpy(), db.coeffs.cpu().numpy(), db.status.cpu().numpy(), db.cost.cpu().numpy()
            assert np.all(st == 1)
            q = _quad(batch, t, 4)
            e = _per_path_error(batch.seg_offsets, c, q["coeffs"])
            errs.append(e)
            above += [(s, int(p), float(e[p])) for p in np.nonzero(e > 1e-8)[0]]
            worst = max(worst, float(e.max()))
            assert np.max(np.abs(cost - q["cost"]) / q["cost"]) < 1e-12, s
    finally:
        plan.close()
    errs = np.concatenate(errs)
    print("REFINE BENCH SLOTS: %d paths, max %.2e, median %.2e, above 1e-11: %d, above 1e-8: %s"
          % (errs.size, worst, np.median(errs), int((errs > TOL_REFINED).sum()), above))
    assert errs.size == SLOTS * PATHS
    assert not above
    assert worst <= TOL_REFINED


def test_fixtures_within_1e_11_of_their_60_digit_coefficients(gpu_ctx, golden):
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_cases.json")) as f:
        cases = golden["cases"] + json.load(f)["cases"]
    rows = []
    for case in cases:
        one, t = util.case_batch(case)
        exact = np.array(case["coeffs"])
        plain = gpu_ctx.solve_batch(one, t)
        got = gpu_ctx.solve_batch(one, t, flags=api.FLAG_REFINE)
        e0, e1 = util.coeff_error(plain["coeffs"], exact), util.coeff_error(got["coeffs"], exact)
        rows.append((case["name"], e0, e1))
        assert np.array_equal(got["status"], plain["status"]) and np.array_equal(got["times"], plain["times"]), case["name"]
        if case["name"] == GUARD_CASE:   # (against its 60 digits: the 113-bit route is 4e-10 off on this path)
            if np.all(np.isfinite(plain["coeffs"])):
                assert np.all(np.isfinite(got["coeffs"])), rows[-1]
            assert e1 <= e0, rows[-1]
            continue
        assert np.all(np.isfinite(got["coeffs"])) and np.isfinite(got["cost"][0]), case["name"]
        assert got["status"][0] == 1, case["name"]
        assert e1 <= TOL_REFINED, rows[-1]
        assert abs(got["cost"][0] - case["cost"]) <= 1e-12 * abs(case["cost"]), case["name"]
    print("REFINE FIXTURES (name, without, with): %s" % ["%s %.1e %.1e" % r for r in rows])


POISON_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
from mrs_uav_trajectory_generation_amd import api
from tests import util
ctx = api.Context(0)
worst = {}
with open(sys.argv[1]) as f:
    cases = [c for c in json.load(f)["cases"] if c["name"] != sys.argv[2]]
for case in cases:
    one, t = util.case_batch(case)
    for _ in range(2):   # (the second call runs on recycled, poisoned blocks as well)
        got = ctx.solve_batch(one, t, flags=api.FLAG_REFINE)
    worst[case["name"]] = util.coeff_error(got["coeffs"], np.array(case["coeffs"]))
print(json.dumps(worst))
"""


def test_a_poisoned_workspace_changes_nothing(gpu_ctx):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", POISON_CHILD % root, os.path.join(root, "tests", "golden", "refine_cases.json"),
                        GUARD_CASE], check=True, cwd=root, timeout=600, capture_output=True, text=True,
                       env=dict(os.environ, MRS_TG_POOL_POISON="1"))
    worst = json.loads(r.stdout.strip().splitlines()[-1])
    print("REFINE POISONED POOL: %s" % worst)
    for name in ("ratio50_d3", "ratio100_d3", "ratio50_d2", "ratio100_d2", "free_end_derivatives", "ratio100_d4"):
        assert worst[name] <= TOL_REFINED, (name, worst[name])
    assert max(worst.values()) <= TOL_REFINED, worst


def _mode_pair(ctx, batch, mode, flags_extra=0):
    kw = dict(time_alloc_method=mode, sampling_dt=0.0)
    plain = ctx.solve_batch(batch, None, flags=flags_extra, **kw)
    ref = ctx.solve_batch(batch, None, flags=flags_extra | api.FLAG_REFINE, **kw)
    return plain, ref


@pytest.mark.parametrize("mode,n_seg,n_paths", [(api.TIME_ALLOC_MELLINGER, 10, 1024), (api.TIME_ALLOC_SQUARED_TIME, 10, 1024),
                                                (api.TIME_ALLOC_MELLINGER, "ragged", 8192)])
def test_time_allocation_modes_keep_times_and_status_and_refine_the_final_solve(gpu_ctx, mode, n_seg, n_paths):
    batch = pr.random_batch(n_paths, n_seg, seed0=31000)
    plain, ref = _mode_pair(gpu_ctx, batch, mode)
    assert np.array_equal(ref["times"], plain["times"])
    assert np.array_equal(ref["status"], plain["status"])
    so = batch.seg_offsets
    q = _quad(batch, ref["times"], batch.derivative_to_optimize)
    ok = ref["status"] > 0
    e1 = _per_path_error(so, ref["coeffs"], q["coeffs"])
    e0 = _per_path_error(so, plain["coeffs"], q["coeffs"])
    hard = _neighbour_cond(so, ref["times"], batch.derivative_to_optimize) > GUARD_REGIME_COND
    easy = ok & ~hard
    print("REFINE MODE %d %s x %d: %d paths status > 0 (%d in the guard regime); max error without %.2e, with %.2e (guard regime: "
          "without %.2e, with %.2e)" % (mode, n_seg, n_paths, int(ok.sum()), int((ok & hard).sum()), e0[easy].max(),
                                        e1[easy].max(), e0[ok & hard].max(initial=0.0), e1[ok & hard].max(initial=0.0)))
    assert easy.sum() > 0.95 * n_paths
    assert e1[easy].max() <= TOL_REFINED, (np.nonzero(e1[easy] > TOL_REFINED)[0][:5], e1[easy].max())
    assert np.all(e1[ok & hard] <= np.maximum(e0[ok & hard], TOL_REFINED))
    assert np.all(np.isfinite(ref["coeffs"][np.repeat(ok, np.diff(so))]))
    # paths the search did not accept keep the solve's coefficients bit for bit
    for p in np.nonzero(~ok)[0]:
        a, b = so[p], so[p + 1]
        assert np.array_equal(ref["coeffs"][a:b], plain["coeffs"][a:b]), p


def test_samples_are_taken_from_the_refined_coefficients(gpu_ctx):
    batch = pr.random_batch(256, 10, seed0=32000)
    dt, cap = 0.05, 4096
    out = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, sampling_dt=dt, sample_capacity=cap,
                              flags=api.FLAG_REFINE)
    plain = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, flags=api.FLAG_REFINE)
    assert np.array_equal(out["coeffs"], plain["coeffs"]) and np.array_equal(out["times"], plain["times"])
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    n_dev = torch.zeros(batch.n_paths, dtype=torch.int32, device="cuda")
    states = torch.zeros((batch.n_paths, cap, api.STATE_ORDERS, 4), dtype=torch.float64, device="cuda")
    plan.sample_states(torch.from_numpy(out["coeffs"]).cuda(), torch.from_numpy(out["times"]).cuda(), dt, cap, n_dev, states)
    torch.cuda.synchronize()
    n_got, st = n_dev.cpu().numpy(), states.cpu().numpy()
    plan.close()
    assert np.array_equal(n_got, out["n_samples"])
    for p in range(batch.n_paths):
        n = min(int(n_got[p]), cap)
        assert np.array_equal(st[p, :n, 0, :], out["samples"][p, :n]), p


def test_find_trajectory_and_optimize_paths_run_the_refinement(gpu_ctx):
    wps = [pr.random_box_waypoints(4 + (i % 5), 33000 + i) for i in range(96)]
    for wp in wps[:6]:
        plain = gpu_ctx.find_trajectory(wp)
        api.kernel_trace_reset()
        got = gpu_ctx.find_trajectory(wp, flags=api.FLAG_REFINE)
        assert "refine_kernel" in api.kernel_trace(), api.kernel_trace()
        assert got["status"] == plain["status"] and got["rejection"] == plain["rejection"]
        assert np.array_equal(got["times"], plain["times"])
    for n in (24, 96):   # fewer than 64 active requests: host rounds; from 64 on: device rounds
        paths = wps[:n]
        plain = api.optimize_paths(gpu_ctx, paths, sample_capacity=4096)
        api.kernel_trace_reset()
        got = api.optimize_paths(gpu_ctx, paths, policy=api.default_policy_options(solver=dict(flags=api.FLAG_REFINE)),
                                 sample_capacity=4096)
        assert "refine_kernel" in api.kernel_trace(), (n, api.kernel_trace())
        assert np.array_equal(got["success"], plain["success"]), n
        assert plain["success"].mean() > 0.9


def test_two_identical_calls_give_identical_bits(gpu_ctx):
    batch = pr.random_batch(2048, "ragged", seed0=34000)
    a = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, flags=api.FLAG_REFINE)
    b = gpu_ctx.solve_batch(batch, None, time_alloc_method=api.TIME_ALLOC_MELLINGER, flags=api.FLAG_REFINE)
    for k in ("times", "coeffs", "status", "cost"):
        assert np.array_equal(a[k], b[k]), k


def test_explain_names_the_refinement_and_grouped_launches_refuse_it(gpu_ctx):
    batch = pr.random_batch(1024, 10, seed0=35000)
    plan = api.Plan(gpu_ctx, batch.seg_offsets)
    try:
        for mode in (api.TIME_ALLOC_NONE, api.TIME_ALLOC_MELLINGER, api.TIME_ALLOC_SQUARED_TIME):
            base = plan.explain(api.default_options(time_alloc_method=mode))
            with_flag = plan.explain(api.default_options(time_alloc_method=mode, flags=api.FLAG_REFINE))
            assert "refine_kernel" not in base
            # (explain reports the newest 32 launches: a gradient-free search launches more, so compare the tail)
            assert with_flag == (base + ["refine_kernel"])[-32:], (mode, base, with_flag)
        with pytest.raises(api.MrsTgError) as ei:
            plan.explain(api.default_options(flags=api.FLAG_REFINE), group_size=2)
        assert "MRS_TG_FLAG_REFINE" in str(ei.value)
        db = api.DeviceBatch(batch, "cuda:0")
        t = torch.from_numpy(util.oracle_times(batch)).cuda()
        db.seg_times.copy_(t)
        call = plan.bind_solve(api.default_options(flags=api.FLAG_REFINE), db.fixed_mask, db.fixed_values, db.seg_times, db.coeffs,
                               db.status, db.cost)
        with pytest.raises(api.MrsTgError) as ei:
            api.RoundRobin([call, call], grouped=True)(2)
        assert "MRS_TG_FLAG_REFINE" in str(ei.value)
        call()   # the same bound solve launched on its own is refined
        torch.cuda.synchronize()
        q = _quad(batch, db.seg_times.cpu().numpy(), 4)
        assert _per_path_error(batch.seg_offsets, db.coeffs.cpu().numpy(), q["coeffs"]).max() <= TOL_REFINED
    finally:
        plan.close()

"""The backward pass of the fixed-times solve on the CPU: the per-lane routine of csrc/mrs_tg_vjp.hpp (the one vjp_kernel runs),
compiled with g++ by tests/host/vjp_harness.cpp, against

  * the 60-digit central differences of tests/golden/vjp_cases.json (gen_vjp_cases.py): every well-conditioned case to 1e-10
    of the path's largest gradient entry, the ill-conditioned one (a segment 50 times shorter than its neighbours) to the bound
    this harness measures, the 30-segment path along its three directions;
  * those of tests/golden/vjp_edge_cases.json (gen_vjp_cases.py --edges) to the same 1e-10: one and two segments, d = 0 and 1,
    position-only end and start vertices, no free slot at all, a fixed slot between free ones, adjacent position-free and
    adjacent stop_at vertices;
  * a dense float64 torch-autograd restatement (tests/vjp_util.py) on 200 random paths;
  * itself under -fsanitize=address,undefined (host code only).

The harness fills its workspace and outputs with NaNs before every lane: a NaN in a result means the routine read an element
it had not written, or left an output unwritten."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import problem as pr
from tests import vjp_util as vu

TOL_WELL = 1e-10
ILL_CASE = "ratio50"
TOL_ILL = 1e-5        # measured 3.2e-6 (cond(R_pp) ~ 50^7 between the short segment and its neighbours)
TOL_TORCH_MAX, TOL_TORCH_MEDIAN = 1e-6, 1e-8   # the restatement's own error dominates (dense solve of the unscaled KKT system)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return vu.build_harness(tmp_path_factory.mktemp("vjp"))


def _fixture_errors(results, cases):
    out = {}
    for case, (gv, gt) in zip(cases, results):
        assert np.all(np.isfinite(gv)) and np.all(np.isfinite(gt)), case["name"]
        if "directions" in case:
            out[case["name"]] = vu.directional_error(case, gv, gt)
        else:
            out[case["name"]] = vu.rel_error(gv, gt, np.array(case["grad_fixed_values"]), np.array(case["grad_seg_times"]))
    return out


def test_fixtures_hold_the_required_cases():
    cases = vu.load_cases()
    names = {c["name"] for c in cases}
    assert {"free_end_stop_at", "position_free_vertex", ILL_CASE, "seg30_directional"} <= names
    assert {c["derivative_to_optimize"] for c in cases} == {2, 3, 4}
    for c in cases:
        m = np.array(c["fixed_mask"])
        assert 3 <= len(c["seg_times"]) <= 6 or "directions" in c, c["name"]
        g = np.array(c["grad_coeffs"])
        assert np.array_equal(g * 64, np.round(g * 64)) and c["grad_cost"] * 8 == round(c["grad_cost"] * 8)   # dyadic
        if "directions" not in c:   # free slots carry no gradient
            assert np.all(np.array(c["grad_fixed_values"])[m == 0] == 0.0), c["name"]
    free_end = next(c for c in cases if c["name"] == "free_end_stop_at")
    assert np.array(free_end["fixed_mask"])[-1].tolist() == [1, 0, 0, 0, 0]
    assert np.array(next(c for c in cases if c["name"] == "position_free_vertex")["fixed_mask"])[2, 0] == 0
    assert len(next(c for c in cases if c["name"] == "seg30_directional")["seg_times"]) == 30
    # the edge file (gen_vjp_cases.py --edges): the lengths and derivatives the file above leaves out, and its patterns
    edges = {c["name"]: c for c in vu.load_edge_cases()}
    assert not set(edges) & names
    key = {(c["derivative_to_optimize"], len(c["seg_times"])) for c in edges.values()}
    assert {(4, 1), (2, 1), (4, 2), (3, 2), (1, 3), (0, 3), (0, 1)} <= key
    assert {d for d, _ in key} == {0, 1, 2, 3, 4} and {S for _, S in key} == {1, 2, 3, 4}
    for c in edges.values():
        m = np.array(c["fixed_mask"])
        assert "directions" not in c and m.shape == (len(c["seg_times"]) + 1, 5), c["name"]
        g = np.array(c["grad_coeffs"])
        assert np.array_equal(g * 64, np.round(g * 64)) and c["grad_cost"] * 8 == round(c["grad_cost"] * 8)   # dyadic
        assert np.all(np.array(c["grad_fixed_values"])[m == 0] == 0.0), c["name"]
        assert np.any(np.array(c["grad_seg_times"]) != 0.0), c["name"]

    def mask(name):
        return np.array(edges[name]["fixed_mask"])
    assert len(edges["s1_free_end"]["seg_times"]) == 1 and mask("s1_free_end")[-1].tolist() == [1, 0, 0, 0, 0]
    assert len(edges["s3_free_start"]["seg_times"]) == 3 and mask("s3_free_start")[0].tolist() == [1, 0, 0, 0, 0]
    assert len(edges["s3_all_fixed"]["seg_times"]) == 3 and np.all(mask("s3_all_fixed") == 1)
    assert np.any(np.array(edges["s3_all_fixed"]["grad_fixed_values"])[1:-1, 1:] != 0.0)
    assert mask("s4_fixed_acc_free_vel")[1].tolist() == [1, 0, 1, 0, 0]
    assert mask("s4_two_position_free")[1:3, 0].tolist() == [0, 0]
    assert mask("s4_two_stop_at")[1:3].tolist() == [[1, 1, 1, 1, 0]] * 2
    for name in ("d1_s3", "d0_s3", "d0_s1"):   # built for d = 2: the end vertices fix position, velocity and acceleration
        assert mask(name)[0].tolist() == mask(name)[-1].tolist() == [1, 1, 1, 0, 0], name


def test_lane_routine_matches_every_fixture(harness):
    cases = vu.load_cases() + vu.load_edge_cases()
    errs = _fixture_errors(vu.run_harness(harness, [vu.case_problem(c) for c in cases]), cases)
    print("VJP HOST FIXTURES: %s" % {k: "%.1e" % v for k, v in errs.items()})
    for name, e in errs.items():
        assert e <= (TOL_ILL if name == ILL_CASE else TOL_WELL), (name, e)


def test_null_upstream_coefficients_count_as_zero(harness):
    cases = [c for c in vu.load_cases() + vu.load_edge_cases() if "directions" not in c]
    nul = [dict(vu.case_problem(c), G=None) for c in cases]
    zero = [dict(vu.case_problem(c), G=np.zeros_like(np.array(c["grad_coeffs"]))) for c in cases]
    for (a_v, a_t), (b_v, b_t) in zip(vu.run_harness(harness, nul), vu.run_harness(harness, zero)):
        assert np.array_equal(a_v, b_v) and np.array_equal(a_t, b_t)
        assert np.all(np.isfinite(a_v)) and np.any(a_t != 0.0)


def _random_problems(n_paths, seed):
    """n_paths paths in groups of one (d, S): Euclidean times, random stop_at / free end derivatives, Gaussian G and g"""
    from tests import util
    rng = np.random.default_rng(seed)
    groups = []
    per = 20
    for gi in range(n_paths // per):
        d, S = (2, 3, 4)[gi % 3], 3 + gi % 6
        parts = []
        for p in range(per):
            stop = [bool(rng.integers(0, 4) == 0) for _ in range(S + 1)]
            wp, m, v = pr.build_vertices(pr.random_box_waypoints(S, seed + 1000 * gi + p), d, stop_at=stop)
            if rng.integers(0, 3) == 0:
                m[-1, 1:] = 0
                v[-1, 1:, :] = 0.0
            parts.append((wp, m, v))
        batch = pr.assemble_batch(parts, np.tile(pr.DEFAULT_LIMITS, (per, 1)), d)
        t = util.oracle_times(batch).reshape(per, S)
        groups.append((d, S, batch.fixed_mask.reshape(per, S + 1, 5), batch.fixed_values.reshape(per, S + 1, 5, 4), t,
                       rng.standard_normal((per, S, 4, 10)), rng.standard_normal(per)))
    return groups


def test_lane_routine_matches_a_dense_torch_restatement_on_200_random_paths(harness):
    errs = []
    for d, S, m, v, t, G, g in _random_problems(200, 4242):
        C, J, gv, gt = vu.dense_vjp(m, v, t, d, G, g)
        probs = [dict(d=d, mask=m[p], vals=v[p], times=t[p], coeffs=C[p], G=G[p], g=g[p]) for p in range(len(t))]
        for p, (hv, ht) in enumerate(vu.run_harness(harness, probs)):
            assert np.all(hv[m[p] == 0] == 0.0)
            errs.append(vu.rel_error(hv, ht, gv[p], gt[p]))
    errs = np.array(errs)
    print("VJP HOST vs TORCH: %d paths, max %.2e, median %.2e" % (errs.size, errs.max(), np.median(errs)))
    assert errs.size == 200
    assert errs.max() <= TOL_TORCH_MAX and np.median(errs) <= TOL_TORCH_MEDIAN


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = vu.build_harness(tmp_path, sanitize=True)
    cases = vu.load_cases() + vu.load_edge_cases()
    probs = [vu.case_problem(c) for c in cases] + [dict(vu.case_problem(c), G=None) for c in (cases[0], cases[-1])]
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    got = vu.run_harness(san, probs, env=env)
    ref = vu.run_harness(harness, probs)
    for (a_v, a_t), (b_v, b_t) in zip(got, ref):
        assert np.array_equal(a_v, b_v) and np.array_equal(a_t, b_t)

"""The backward pass of the segment maxima on the CPU: the per-entry routine and segment sums of csrc/mrs_tg_maxima_vjp.hpp (the
ones segment_maxima_vjp_kernel runs), compiled with g++ by tests/host/maxima_vjp_harness.cpp, against the 60-digit central
differences of tests/golden/maxima_vjp_cases.json (gen_maxima_vjp_cases.py):

  * seeded 3e-7 T to either side of the fixture's maximiser (the forward search's stopping accuracy), the refinement gives t*
    to 1e-12 T and every entry's gradients to 1e-10 of its largest component; end points are seeded exactly (the search's
    grid holds them) and are not moved;
  * the tie case gives the one-sided gradient of the peak it was seeded at;
  * a refinement that would leave the seed's grid cell, or move further than 2^-20, is refused (the gradient is taken at the
    seed); one whose m2 comes out lower only by rounding is kept;
  * zero upstream entries contribute exactly 0, zero maxima give finite zeros, T <= 0 and non-finite inputs give zero rows;
  * itself under -fsanitize=address,undefined (host code only).

The harness fills its outputs with NaNs first: a NaN in a result means an output element was left unwritten."""
import numpy as np
import pytest

from tests import maxima_vjp_util as mu

TOL_T, TOL_GRAD = 1e-12, 1e-10
SEED_OFFSET = 3e-7


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return mu.build_harness(tmp_path_factory.mktemp("maxima_vjp"))


def _seed_taus(case, sign):
    taus = []
    for e in case["entries"]:
        tau = e["t"] / case["T"]
        taus.append(tau + sign * SEED_OFFSET if 0.0 < tau < 1.0 else tau)
    return taus


def test_fixtures_hold_the_required_cases():
    cases = mu.load_cases()
    names = [c["name"] for c in cases]
    assert {"end_point_maximum", "start_point_maximum", "constant_heading", "rest_to_rest_tie"} <= set(names)
    assert {n.split("_")[1] for n in names if n.startswith("solved_")} == {"d2", "d3", "d4"}
    end = next(c for c in cases if c["name"] == "end_point_maximum")
    assert any(e["t"] == end["T"] and e["grad_T"] != 0.0 for e in end["entries"])
    start = next(c for c in cases if c["name"] == "start_point_maximum")
    assert any(e["t"] == 0.0 and e["maximum"] > 0.0 for e in start["entries"])
    const = next(c for c in cases if c["name"] == "constant_heading")
    assert all(e["maximum"] == 0.0 for e in const["entries"] if e["group"] == 2)
    tie = next(c for c in cases if c["name"] == "rest_to_rest_tie")
    acc_z = next(e for e in tie["entries"] if e["k"] == 2 and e["group"] == 1)
    assert len(acc_z["alternatives"]) == 2 and acc_z["alternatives"][0]["t"] != acc_z["alternatives"][1]["t"]
    for c in cases:   # every other winner is separated from the runner-up (the forward's choice is unambiguous)
        for e in c["entries"]:
            assert "alternatives" in e or e["gap"] is None or e["gap"] >= 1e-3, (c["name"], e["k"], e["group"])


@pytest.mark.parametrize("sign", [1, -1])
def test_refined_maximiser_and_gradients_match_every_fixture(harness, sign):
    cases = mu.load_cases()
    probs = [p for c in cases for p in mu.one_hot_problems(c, _seed_taus(c, sign))]
    res = mu.run_harness(harness, probs)
    worst_t, worst_g = 0.0, 0.0
    for ci, case in enumerate(cases):
        for w, e in enumerate(case["entries"]):
            gc, gT, ts = res[9 * ci + w]
            assert np.all(np.isfinite(gc)) and np.isfinite(gT) and np.all(np.isfinite(ts)), (case["name"], w)
            et = abs(ts[w] - e["t"]) / case["T"]
            eg = mu.entry_error(gc, gT, e) if e["maximum"] > 0.0 else float(np.max(np.abs(gc)) + abs(gT))
            worst_t, worst_g = max(worst_t, et), max(worst_g, eg)
            assert et <= TOL_T, (case["name"], w, et)
            assert eg <= TOL_GRAD, (case["name"], w, eg)
    print("MAXIMA VJP HOST FIXTURES (seed %+g T): t* %.1e T, gradients %.1e" % (sign * SEED_OFFSET, worst_t, worst_g))


def test_the_tie_gives_the_one_sided_gradient_of_the_seeded_peak(harness):
    case = next(c for c in mu.load_cases() if c["name"] == "rest_to_rest_tie")
    w = next(i for i, e in enumerate(case["entries"]) if "alternatives" in e)
    alts = case["entries"][w]["alternatives"]
    got = []
    for alt in alts:
        taus = _seed_taus(case, 1)
        taus[w] = alt["t"] / case["T"] + SEED_OFFSET
        gc, gT, ts = mu.run_harness(harness, mu.one_hot_problems(case, taus))[w]
        assert abs(ts[w] - alt["t"]) <= TOL_T * case["T"]
        assert mu.entry_error(gc, gT, alt) <= TOL_GRAD
        got.append(gc)
    assert not np.allclose(got[0], got[1])   # the two one-sided gradients differ: the entry is not differentiable there


REACH = 2.0 ** -20   # kRefineReach, mrs_tg_maxima_vjp.hpp


def _interior_entry(name_prefix):
    case = next(c for c in mu.load_cases() if c["name"].startswith(name_prefix))
    w = next(i for i, e in enumerate(case["entries"]) if 0.1 < e["t"] / case["T"] < 0.9 and e["gap"] is not None)
    return case, w, case["entries"][w]["t"] / case["T"]


def _seeded(harness, case, w, seed, lo, hi):
    p = mu.one_hot_problems(case, _seed_taus(case, 1))[w]
    p["seeds"][w] = (seed, lo, hi, 1.0)
    gc, gT, ts = mu.run_harness(harness, [p])[0]
    return gc, gT, ts[w] / case["T"]


def test_a_refinement_that_leaves_the_seed_cell_is_refused(harness):
    # a move well inside the reach (3e-7 < 2^-20) whose end lies outside the given cell: only the cell test refuses it
    case, w, tau = _interior_entry("solved_d3")
    seed = tau + SEED_OFFSET
    _, _, inside = _seeded(harness, case, w, seed, tau - 1e-6, tau + 1e-6)
    _, _, outside = _seeded(harness, case, w, seed, tau + 1e-7, tau + 1e-6)
    assert abs(inside - tau) <= TOL_T and abs(seed - tau) <= REACH
    assert outside == seed * case["T"] / case["T"]   # kept at the seed


def test_a_refinement_that_moves_beyond_its_reach_is_refused(harness):
    # the same maximum seeded 2e-6 away inside one wide cell: Newton gets there, the reach guard (2^-20) refuses the move
    case, w, tau = _interior_entry("solved_d3")
    near, far = tau + 0.5 * REACH, tau + 2.0 * REACH
    _, _, a = _seeded(harness, case, w, near, tau - 0.01, tau + 0.01)
    _, _, b = _seeded(harness, case, w, far, tau - 0.01, tau + 0.01)
    assert abs(a - tau) <= TOL_T
    assert b == far * case["T"] / case["T"]


def test_the_rounding_allowance_keeps_a_refinement_whose_m2_only_rounds_lower(harness):
    # the forward's own winner for this entry (its polish stopped 1.4e-8 from the maximiser): there the refined m2 evaluates
    # 1.2e-14 lower than the seed's, below the rounding of its Horner sum; a strict "did not fall" would keep the seed and a
    # gradient 1e-7 off
    case = next(c for c in mu.load_cases() if c["name"] == "solved_d2_seed71_seg2")
    w = 6
    e = case["entries"][w]
    gc, gT, t = _seeded(harness, case, w, 0.88875429199672118, 0.875, 0.90625)
    assert abs(t - e["t"] / case["T"]) <= TOL_T
    assert mu.entry_error(gc, gT, e) <= TOL_GRAD


def test_zero_upstream_zero_maximum_and_unusable_segments(harness):
    cases = mu.load_cases()
    const = next(c for c in cases if c["name"] == "constant_heading")
    taus = _seed_taus(const, 1)
    # all upstream 0: exactly 0 everywhere
    zero = dict(coeffs=const["coeffs"], T=const["T"], seeds=[(t, *mu.cell_of(t), 0.0) for t in taus])
    # upstream only on the zero-maximum heading entries: finite zeros
    heading = dict(coeffs=const["coeffs"], T=const["T"],
                   seeds=[(t, *mu.cell_of(t), 1.0 if w % 3 == 2 else 0.0) for w, t in enumerate(taus)])
    bad = []
    for T in (0.0, -1.0, float("nan"), float("inf")):
        bad.append(dict(coeffs=const["coeffs"], T=T, seeds=[(t, *mu.cell_of(t), 1.0) for t in taus]))
    c = np.array(const["coeffs"])
    c[1, 4] = float("nan")
    bad.append(dict(coeffs=c, T=const["T"], seeds=[(t, *mu.cell_of(t), 1.0) for t in taus]))
    res = mu.run_harness(harness, [zero, heading] + bad)
    for gc, gT, _ in res[:2]:
        assert np.all(gc == 0.0) and gT == 0.0
    for gc, gT, ts in res[2:]:
        assert np.all(gc == 0.0) and gT == 0.0 and np.all(ts == 0.0)


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = mu.build_harness(tmp_path, sanitize=True)
    cases = mu.load_cases()
    probs = [p for c in cases for p in mu.one_hot_problems(c, _seed_taus(c, 1))]
    probs.append(dict(coeffs=cases[0]["coeffs"], T=0.0, seeds=[(0.5, 0.0, 1.0, 1.0)] * 9))
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    got = mu.run_harness(san, probs, env=env)
    ref = mu.run_harness(harness, probs)
    for (a_c, a_t, a_s), (b_c, b_t, b_s) in zip(got, ref):
        assert np.array_equal(a_c, b_c) and a_t == b_t and np.array_equal(a_s, b_s)

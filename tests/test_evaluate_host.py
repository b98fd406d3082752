"""The evaluation at caller-given times and its backward pass on the CPU: csrc/mrs_tg_evaluate.hpp (the locate rule, the Horner
rows and the per-query terms of evaluate_kernel / evaluate_vjp_kernel) compiled by g++ into tests/host/evaluate_harness.cpp,
against the 60-digit fixtures of tests/golden/gen_evaluate_cases.py and a plain-Python restatement of the locate rule.  No GPU."""
import os

import numpy as np
import pytest

from tests import evaluate_util as eu

TOL_WELL = 1e-10   # the project's bound for well-conditioned backward fixtures (test_vjp_host.py, test_sample_vjp_host.py)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return eu.build_harness(tmp_path_factory.mktemp("evaluate"))


def test_fixtures_hold_the_required_cases():
    grads = {c["name"]: c for c in eu.gradient_cases()}
    fwd = {c["name"]: c for c in eu.forward_cases()}
    assert {"unsorted_duplicate_o5", "empty_segment_o5", "heading_crosses_pi_o5", "seg30_directional"} <= set(grads)
    assert {"forward_edges_o5", "forward_edges_o1", "zero_length_segment_o5"} <= set(fwd)
    assert {c["n_orders"] for c in grads.values()} == {1, 5}
    assert {n.split("_")[0] for n in grads if n[0] == "d" and n[1].isdigit()} == {"d2", "d3", "d4"}
    for c in grads.values():
        Q = len(c["query_times"])
        g = np.array(c["grad_states"])
        assert g.shape == (Q, c["n_orders"], 4) and len(c["query_segment"]) == Q
        assert np.array_equal(g * 64, np.round(g * 64))   # dyadic
        edges = np.concatenate([[0.0], np.cumsum(c["seg_times"])])
        for t, i in zip(c["query_times"], c["query_segment"]):   # every query well inside its segment
            assert edges[i] + 0.9e-6 <= t <= edges[i + 1] - 0.9e-6
        if "directions" not in c:
            assert np.array(c["grad_coeffs"]).shape == (len(c["seg_times"]), 4, 10)
            assert len(c["grad_seg_times"]) == len(c["seg_times"]) and len(c["grad_query_times"]) == Q
            assert c["grad_seg_times"][-1] == 0.0   # the last segment's time moves no query
    q = grads["unsorted_duplicate_o5"]["query_times"]
    assert q != sorted(q) and len(set(q)) == len(q) - 1
    empty = grads["empty_segment_o5"]
    assert 2 not in empty["query_segment"] and {1, 3} <= set(empty["query_segment"])
    assert np.all(np.array(empty["grad_coeffs"])[2] == 0.0) and empty["grad_seg_times"][2] != 0.0
    s30 = grads["seg30_directional"]
    assert len(s30["seg_times"]) == 30 and len(s30["directions"]) == 3
    assert all(len(d["d_query_times"]) == len(s30["query_times"]) for d in s30["directions"])
    edges = fwd["forward_edges_o5"]
    T = edges["seg_times"]
    total = 0.0
    for t in T:
        total += t
    q = edges["query_times"]
    assert q[0] == 0.0 and q[1] == (T[0] + T[1]) and q[2] == total
    assert q[3] == np.nextafter(total, np.inf) and q[4] == np.nextafter(total, -np.inf) and q[5] < 0 and q[6] is None
    assert edges["query_segment"][:7] == [0, 2, len(T) - 1, -1, len(T) - 1, -1, -1]
    zl = fwd["zero_length_segment_o5"]
    assert zl["seg_times"][1] == 0.0 and zl["query_times"][0] == zl["seg_times"][0] and zl["query_segment"][0] == 2
    comp = {c["name"]: c for c in eu.load_composite_cases()}
    assert "ratio50" in comp and len(comp) >= 3
    t = comp["ratio50"]["seg_times"]
    assert t[3] * 40 < min(t[2], t[4])
    assert 3 in comp["ratio50"]["query_segment"]
    for name in ("evaluate_cases.json", "evaluate_composite_cases.json"):
        mine = os.path.getsize(os.path.join(eu.ROOT, "tests", "golden", name))
        assert mine <= os.path.getsize(os.path.join(eu.ROOT, "tests", "golden", name.replace("evaluate", "sample_vjp")))


def test_python_restatement_matches_the_fixtures_segments():
    for c in eu.load_cases():
        for t, i in zip(eu.query_array(c), c["query_segment"]):
            assert eu.locate(c["seg_times"], t)[0] == i, (c["name"], t)


def test_forward_matches_every_forward_fixture(harness):
    cases = eu.forward_cases()
    res = eu.run_harness(harness, [eu.case_problem(c) for c in cases])
    worst = {}
    for c, r in zip(cases, res):
        assert np.array_equal(r["query_segment"], np.array(c["query_segment"])), c["name"]
        out = r["query_segment"] < 0
        assert np.all(r["states"][out] == 0.0) and np.all(r["query_local_time"][out] == 0.0), c["name"]
        assert eu.wrapped_in_range(r["states"]), c["name"]
        worst[c["name"]], ok = eu.forward_error(c, r["states"])
        assert ok, (c["name"], worst[c["name"]])
    print("EVALUATE HOST FORWARD FIXTURES (|err| / largest entry of the order): %s" % {k: "%.1e" % v for k, v in worst.items()})


def test_gradients_match_every_fixture(harness):
    cases = eu.gradient_cases()
    res = eu.run_harness(harness, [eu.case_problem(c) for c in cases])
    errs = {}
    for c, r in zip(cases, res):
        assert np.array_equal(r["query_segment"], np.array(c["query_segment"])), c["name"]
        assert np.max(np.abs(r["query_local_time"] - np.array(c["query_local_time"]))) < 1e-12, c["name"]
        for k in ("grad_coeffs", "grad_seg_times", "grad_query_times"):
            assert np.all(np.isfinite(r[k])), (c["name"], k)
        errs[c["name"]] = eu.fixture_error(c, r["grad_coeffs"], r["grad_seg_times"], r["grad_query_times"])
    print("EVALUATE HOST GRADIENT FIXTURES: %s" % {k: "%.1e" % v for k, v in errs.items()})
    for name, e in errs.items():
        assert e <= TOL_WELL, (name, e)
    empty = next(i for i, c in enumerate(cases) if c["name"] == "empty_segment_o5")
    assert np.all(res[empty]["grad_coeffs"][2] == 0.0) and res[empty]["grad_seg_times"][-1] == 0.0
    dup = next(i for i, c in enumerate(cases) if c["name"] == "unsorted_duplicate_o5")
    assert np.array_equal(res[dup]["states"][0], res[dup]["states"][4])


def _random_paths(n_paths, seed):
    """random paths of 1..12 segments with random, boundary and out-of-range queries; every tenth path has a zero-length
    segment, every 17th a negative time (the sums decrease: the loop, not the bisection), every 23rd a NaN time"""
    rng = np.random.default_rng(seed)
    probs = []
    for p in range(n_paths):
        S = int(rng.integers(1, 13))
        T = rng.uniform(0.05, 3.0, size=S)
        if p % 10 == 3:
            T[int(rng.integers(0, S))] = 0.0
        if p % 17 == 5 and S > 2:
            T[1] = -0.5 * T[0]
        if p % 23 == 7:
            T[int(rng.integers(0, S))] = np.nan
        sums, acc = [], 0.0
        for t in T:
            acc = acc + float(t)
            sums.append(acc)
        total = sums[-1] if sums[-1] == sums[-1] else 10.0
        q = list(rng.uniform(0.0, total, size=20)) + sums + [np.nextafter(s, np.inf) for s in sums] + \
            [np.nextafter(s, -np.inf) for s in sums] + [0.0, -0.0, -1e-300, -1.0, np.nan, np.inf, -np.inf, 2.0 * total,
                                                        np.nextafter(0.0, 1.0)]
        q = np.array(q, dtype=np.float64)
        rng.shuffle(q)
        no = (1, 5)[p % 2]
        probs.append(dict(seg_times=T, coeffs=rng.standard_normal((S, 4, 10)), query_times=q, n_orders=no,
                          grad_states=rng.standard_normal((q.size, no, 4))))
    return probs


def test_locate_matches_the_python_restatement_on_200_random_paths(harness):
    probs = _random_paths(200, 4242)
    res = eu.run_harness(harness, probs)
    n_out = n_in = 0
    for p, r in zip(probs, res):
        for k, t in enumerate(p["query_times"]):
            seg, tau = eu.locate(p["seg_times"], t)
            assert r["query_segment"][k] == seg, (p["seg_times"], t)
            # bit for bit (the harness prints 17 significant digits: the double is recovered exactly)
            assert r["query_local_time"][k] == tau or (tau != tau and r["query_local_time"][k] != r["query_local_time"][k])
            n_out += seg < 0
            n_in += seg >= 0
    print("EVALUATE HOST LOCATE: %d queries in range, %d out of range, all equal" % (n_in, n_out))
    assert n_in > 3000 and n_out > 1000


def test_nan_upstream_on_out_of_range_rows_changes_no_bit(harness):
    probs = [p for p in _random_paths(40, 77) if not np.any(np.isnan(p["seg_times"]))]
    clean = eu.run_harness(harness, probs)
    dirty = []
    for p, r in zip(probs, clean):
        G = np.array(p["grad_states"])
        assert np.any(r["query_segment"] < 0)
        G[r["query_segment"] < 0] = np.nan
        dirty.append(dict(p, grad_states=G))
    for a, b in zip(eu.run_harness(harness, dirty), clean):
        assert a["raw"] == b["raw"]
        assert np.all(np.isfinite(a["grad_coeffs"])) and np.all(np.isfinite(a["grad_query_times"]))
        assert np.all(a["grad_query_times"][a["query_segment"] < 0] == 0.0)


def test_status_below_one_gives_zero_rows(harness):
    case = eu.gradient_cases()[0]
    bad = eu.case_problem(case, status=-2, coeffs=np.full_like(np.array(case["coeffs"]), np.nan))
    r = eu.run_harness(harness, [bad])[0]
    assert np.all(r["grad_coeffs"] == 0.0) and np.all(r["grad_seg_times"] == 0.0) and np.all(r["grad_query_times"] == 0.0)


def test_no_queries_gives_zero_gradients(harness):
    case = eu.gradient_cases()[0]
    r = eu.run_harness(harness, [eu.case_problem(case, query_times=np.zeros(0), grad_states=np.zeros((0, case["n_orders"], 4)))])[0]
    assert np.all(r["grad_coeffs"] == 0.0) and np.all(r["grad_seg_times"] == 0.0) and r["grad_query_times"].size == 0


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = eu.build_harness(tmp_path, sanitize=True)
    probs = [eu.case_problem(c) for c in eu.load_cases()] + _random_paths(30, 5)
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    got = eu.run_harness(san, probs, env=env)
    ref = eu.run_harness(harness, probs)
    for a, b in zip(got, ref):
        assert a["raw"] == b["raw"]

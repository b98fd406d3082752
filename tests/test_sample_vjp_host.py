"""The backward pass of the sampler on the CPU: csrc/mrs_tg_sample_vjp.hpp (the per-term routines and sums of
sample_vjp_kernel) compiled by g++ into tests/host/sample_vjp_harness.cpp, against the 60-digit fixtures of
tests/golden/gen_sample_vjp_cases.py and against torch autograd of a dense Horner restatement.  No GPU."""
import numpy as np
import pytest
import torch

from mrs_uav_trajectory_generation_amd import problem as pr
from tests import sample_vjp_util as su
from tests import util

TOL_WELL = 1e-10   # the project's bound for well-conditioned backward fixtures (test_vjp_host.py)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return su.build_harness(tmp_path_factory.mktemp("sample_vjp"))


def test_fixtures_hold_the_required_cases():
    cases = su.load_cases()
    by_name = {c["name"]: c for c in cases}
    assert {"short_segment_no_sample_o5", "one_sample_segment_o1", "heading_crosses_pi_o5", "overflow_o5",
            "seg30_directional"} <= set(by_name)
    assert {c["n_orders"] for c in cases} == {1, 5}
    assert len({c["dt"] for c in cases}) >= 2 and 0.2 in {c["dt"] for c in cases}
    for c in cases:
        assert 3 <= len(c["seg_times"]) <= 6 or "directions" in c, c["name"]
        g = np.array(c["grad_states"])
        assert g.shape == (min(c["n_samples"], c["capacity"]), c["n_orders"], 4)
        assert np.array_equal(g * 64, np.round(g * 64))   # dyadic
    short = by_name["short_segment_no_sample_o5"]
    assert short["seg_times"][2] < short["dt"] and 2 not in short["sample_segment"]
    assert {1, 3} <= set(short["sample_segment"])
    assert np.all(np.array(short["grad_coeffs"])[2] == 0.0) and short["grad_seg_times"][2] != 0.0
    assert by_name["one_sample_segment_o1"]["sample_segment"].count(2) == 1
    over = by_name["overflow_o5"]
    assert over["n_samples"] == over["capacity"] + 1 and over["n_exact"] > over["capacity"]
    assert len(by_name["seg30_directional"]["seg_times"]) == 30 and len(by_name["seg30_directional"]["directions"]) == 3
    for c in cases:   # the last segment's time moves no sample
        if "directions" not in c:
            assert c["grad_seg_times"][-1] == 0.0
    comp = {c["name"]: c for c in su.load_composite_cases()}
    assert "ratio50" in comp
    t = comp["ratio50"]["seg_times"]
    assert t[3] * 40 < min(t[2], t[4])


def test_routine_matches_every_fixture(harness):
    cases = su.load_cases()
    res = su.run_harness(harness, [su.case_problem(c) for c in cases])
    errs = {}
    for c, r in zip(cases, res):
        assert r["n"] == c["n_samples"], c["name"]
        assert np.array_equal(r["sample_segment"], np.array(c["sample_segment"])), c["name"]
        assert np.max(np.abs(r["sample_time"] - np.array(c["sample_time"]))) < 1e-12, c["name"]
        assert np.all(np.isfinite(r["grad_coeffs"])) and np.all(np.isfinite(r["grad_seg_times"])), c["name"]
        errs[c["name"]] = su.fixture_error(c, r["grad_coeffs"], r["grad_seg_times"])
    print("SAMPLE VJP HOST FIXTURES: %s" % {k: "%.1e" % v for k, v in errs.items()})
    for name, e in errs.items():
        assert e <= TOL_WELL, (name, e)
    short = next(i for i, c in enumerate(cases) if c["name"] == "short_segment_no_sample_o5")
    assert np.all(res[short]["grad_coeffs"][2] == 0.0) and res[short]["grad_seg_times"][-1] == 0.0


def test_overflow_reads_nothing_beyond_the_capacity(harness):
    case = next(c for c in su.load_cases() if c["name"] == "overflow_o5")
    plain = su.run_harness(harness, [su.case_problem(case)])[0]
    padded = su.run_harness(harness, [su.case_problem(case, pad_rows=case["n_exact"] - case["capacity"] + 2)])[0]
    assert plain["n"] == padded["n"] == case["capacity"] + 1
    assert np.all(np.isfinite(padded["grad_coeffs"])) and np.all(np.isfinite(padded["grad_seg_times"]))
    assert plain["raw"] == padded["raw"]


def test_status_below_one_gives_zero_rows(harness):
    case = su.load_cases()[0]
    bad = dict(su.case_problem(case), status=-2, coeffs=np.full_like(np.array(case["coeffs"]), np.nan))
    r = su.run_harness(harness, [bad])[0]
    assert r["n"] == case["n_samples"]
    assert np.all(r["grad_coeffs"] == 0.0) and np.all(r["grad_seg_times"] == 0.0)


def _random_solved_paths(n_paths, seed):
    """n_paths solved paths of 3..8 segments at d = 2, 3, 4 (the oracle's linear solve at Euclidean times)"""
    out = []
    per = 25
    for gi in range(n_paths // per):
        d, S = (2, 3, 4)[gi % 3], 3 + gi % 6
        batch = pr.random_batch(per, S, seed0=seed + 1000 * gi, derivative_to_optimize=d)
        t = util.oracle_times(batch)
        ref = util.oracle_linear(batch, t)
        assert np.all(ref["status"] > 0)
        for p in range(per):
            out.append((ref["coeffs"][p * S:(p + 1) * S], t[p * S:(p + 1) * S]))
    return out


def test_routine_matches_torch_autograd_of_a_dense_horner_on_200_random_paths(harness):
    rng = np.random.default_rng(99)
    paths = _random_solved_paths(200, 31000)
    probs = []
    for q, (c, t) in enumerate(paths):
        no = (1, 5)[q % 2]
        dt = (0.2, 0.13, 0.31)[q % 3]
        cap = int(np.sum(t) / dt) + 8
        probs.append(dict(seg_times=t, coeffs=c, dt=dt, capacity=cap, n_orders=no, grad_states=rng.standard_normal((cap, no, 4))))
    res = su.run_harness(harness, probs)
    errs = []
    for p, r in zip(probs, res):
        n = r["n"]
        assert 0 < n <= p["capacity"]
        c = torch.tensor(p["coeffs"], dtype=torch.float64, requires_grad=True)
        T = torch.tensor(p["seg_times"], dtype=torch.float64, requires_grad=True)
        seg = torch.from_numpy(r["sample_segment"])
        tk = su.sample_times_expr(torch, T, [0, len(p["seg_times"])], torch.zeros(n, dtype=torch.int64), seg, torch.arange(n), p["dt"])
        assert float(torch.max(torch.abs(tk.detach() - torch.from_numpy(r["sample_time"])))) < 1e-11
        st = su.states_at(torch, c, seg, tk, p["n_orders"])
        (st * torch.from_numpy(p["grad_states"][:n])).sum().backward()
        gc, gt = c.grad.numpy(), T.grad.numpy()
        scale = max(np.max(np.abs(gc)), np.max(np.abs(gt)))
        errs.append(max(np.max(np.abs(r["grad_coeffs"] - gc)), np.max(np.abs(r["grad_seg_times"] - gt))) / scale)
    errs = np.array(errs)
    print("SAMPLE VJP HOST vs TORCH: %d paths, max %.2e, median %.2e" % (errs.size, errs.max(), np.median(errs)))
    assert errs.size == 200 and errs.max() <= TOL_WELL


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = su.build_harness(tmp_path, sanitize=True)
    cases = su.load_cases()
    over = next(c for c in cases if c["name"] == "overflow_o5")
    probs = [su.case_problem(c) for c in cases] + [su.case_problem(over, pad_rows=3), dict(su.case_problem(cases[0]), status=0)]
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    got = su.run_harness(san, probs, env=env)
    ref = su.run_harness(harness, probs)
    for a, b in zip(got, ref):
        assert a["raw"] == b["raw"]

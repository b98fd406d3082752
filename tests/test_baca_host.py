"""The Baca segment-time estimate as a plan step, its backward pass and the length gate on the CPU: csrc/mrs_tg_baca.hpp (the
forward with its flags, the partials and the sums of baca_times_kernel, baca_times_vjp_kernel and length_gate_kernel) compiled
by g++ into tests/host/baca_harness.cpp, against the 60-digit fixtures of tests/golden/gen_baca_cases.py, against the oracle's
and the library's host estimator, and against a restatement of the gate.  No GPU."""
import os

import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api, build
from oracle import pyoracle as po
from tests import baca_util as bu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return bu.build_harness(tmp_path_factory.mktemp("baca"))


@pytest.fixture(scope="module")
def fixture_results(harness):
    cases = bu.load_cases()
    return cases, bu.run_harness(harness, [bu.case_problem(c) for c in cases])


@pytest.fixture(scope="module")
def groups():
    """the fixture's paths and the four batches of the GPU tier, as harness problems"""
    out = dict(fixture=[bu.case_problem(c) for c in bu.load_cases()])
    for n, (name, batch) in enumerate(bu.shapes().items()):
        out[name] = bu.batch_problems(batch, 10 + n)
    return out


def test_fixture_holds_the_required_cases():
    cases = {c["name"]: c for c in bu.load_cases()}
    S = {name: len(c["flags"]) for name, c in cases.items()}
    assert {1, 2, 3, 4, 7} <= set(S.values())
    regime = lambda n: [f & 7 for f in cases[n]["flags"]]   # noqa: E731
    assert regime("v_alone_vertical")[0] == bu.V_VERTICAL and regime("a_alone_vertical")[0] == bu.A_VERTICAL
    assert regime("j_alone_vertical")[0] == bu.J_VERTICAL
    w = np.array(cases["right_angle"]["waypoints"])[:, :3]
    assert np.dot(w[1] - w[0], w[2] - w[1]) == 0.0 and not any(f & (bu.DOT1_CLAMPED | bu.DOT2_CLAMPED) for f in cases["right_angle"]["flags"])
    assert cases["reversal"]["flags"][0] & bu.DOT2_CLAMPED and cases["reversal"]["flags"][1] & bu.DOT1_CLAMPED
    w = np.array(cases["straight_corner"]["waypoints"])[:, :3]
    assert np.array_equal(w[2] - w[1], w[1] - w[0])
    caps = bu.T1_CAPPED | bu.T2_CAPPED
    assert cases["both_caps"]["flags"][0] & caps == caps and cases["one_cap_only"]["flags"][0] & caps == bu.T1_CAPPED
    assert not any(f & caps for f in cases["no_cap"]["flags"])
    w = np.array(cases["coincident_in_the_middle"]["waypoints"])
    assert np.array_equal(w[1], w[2]) and cases["coincident_in_the_middle"]["flags"][1] & (bu.FLOOR | bu.HEADING) == bu.FLOOR
    w = np.array(cases["coincident_at_the_end"]["waypoints"])
    assert np.array_equal(w[-1], w[-2]) and cases["coincident_at_the_end"]["flags"][-1] & (bu.FLOOR | bu.HEADING) == bu.FLOOR
    w = np.array(cases["five_millimetres"]["waypoints"])[:, :3]
    assert abs(np.linalg.norm(w[2] - w[1]) - 0.005) < 1e-12 and cases["five_millimetres"]["flags"][1] & (bu.FLOOR | bu.HEADING) == bu.FLOOR
    heading = {(bool(f & bu.HEADING_CRUISE), bool(f & bu.HEADING_ACC)) for c in cases.values() for f in c["flags"] if f & bu.HEADING}
    assert heading == {(False, False), (True, False), (False, True), (True, True)}
    assert [r[3] for r in cases["seam"]["waypoints"]] == [3.1, -3.1] and cases["seam"]["flags"][0] & bu.HEADING
    assert [r[3] for r in cases["seam_the_other_way"]["waypoints"]] == [-3.1, 3.1] and cases["seam_the_other_way"]["flags"][0] & bu.HEADING
    assert cases["relaxed_heading"]["limits"][2] == bu.FLT_MAX
    assert not any(f & (bu.HEADING | bu.HEADING_CRUISE | bu.HEADING_ACC) for f in cases["relaxed_heading"]["flags"])
    drawn = [c for n, c in cases.items() if n.startswith("limits_drawn")]
    assert len(drawn) >= 3 and all(0.3 <= v <= 4.0 for c in drawn for v in c["limits"])
    seen = 0
    for c in cases.values():
        for f in c["flags"]:
            seen |= f
        g = np.array(c["upstream"])
        assert np.array_equal(g * 64, np.round(g * 64)) and np.all(np.abs(g) <= 1.0)   # dyadic, at most 1
        assert np.array(c["grad_waypoints"]).shape == (len(c["waypoints"]), 4) and len(c["grad_limits"]) == 9
        assert c["grad_limits"][8] == 0.0
    assert seen == 2047   # every bit of MRS_TG_BACA_*
    assert os.path.getsize(bu.FIXTURES) < 100 * 1024


def test_flags_are_the_fixtures(fixture_results):
    for c, r in zip(*fixture_results):
        assert r["flags"].tolist() == c["flags"], c["name"]


def test_values_match_60_digits_to_1e_13(fixture_results):
    worst = 0.0
    for c, r in zip(*fixture_results):
        exact = np.array(c["value"])
        err = np.abs(r["value"] - exact) / exact
        worst = max(worst, float(err.max()))
        assert np.all(err <= bu.VALUE_RTOL), (c["name"], err)
        floor = (np.array(c["flags"]) & (bu.FLOOR | bu.HEADING)) == bu.FLOOR
        assert np.all(r["value"][floor] == 0.01)
    print("BACA HOST VALUES: worst relative error %.2e, %.3f of the bound" % (worst, worst / bu.VALUE_RTOL))


def test_gradients_match_every_fixture_within_the_derived_bound(fixture_results):
    report = {}
    for c, r in zip(*fixture_results):
        ew, el, ratio = bu.gradient_excess(c, r["grad_waypoints"], r["grad_limits"])
        report[c["name"]] = "%.3f" % ratio
        assert ew <= 0.0 and el <= 0.0, (c["name"], ew, el)
        assert r["grad_limits"][8] == 0.0, c["name"]
    print("BACA HOST GRADIENT FIXTURES, largest |error| / bound: %s" % report)
    print("BACA HOST GRADIENT FIXTURES, worst ratio %.3f" % max(float(v) for v in report.values()))


def test_values_agree_with_the_oracle_and_with_the_librarys_host_estimate(harness, groups):
    build.build()
    seen = 0
    for name, probs in groups.items():
        for p, r in zip(probs, bu.run_harness(harness, probs)):
            ref = po.estimate_times(p["waypoints"], p["limits"], baca=True)
            host = api.estimate_times_baca(p["waypoints"], p["limits"])
            assert np.all(np.abs(r["value"] - ref) <= bu.VALUE_RTOL * ref), name
            assert np.all(np.abs(r["value"] - host) <= bu.VALUE_RTOL * host), name
            for f in r["flags"]:
                seen |= int(f)
    assert seen == 2047


def test_every_segment_of_the_gpu_batches_keeps_its_distance_from_the_branch_boundaries(harness, groups):
    """the harness's smallest relative margin to a comparison of the forward that could go the other way: 1e-9 is seven orders
    above what libm and the device's atan2 / sin / cos can differ by, so the flags cannot differ between them on these batches"""
    for name, probs in groups.items():
        if name == "fixture":
            continue
        worst = min(float(r["margin"].min()) for r in bu.run_harness(harness, probs))
        print("BACA MARGIN %s: %.3g" % (name, worst))
        assert worst >= bu.MARGIN, (name, worst)


def _one_hot_contributions(harness, p):
    """the problem once per segment with the other upstream entries zeroed: each run's outputs are one segment's own parts
    (0.0 + x = x exactly)"""
    S = len(p["upstream"])
    runs = [dict(p, upstream=np.where(np.arange(S) == j, p["upstream"], 0.0)) for j in range(S)]
    return bu.run_harness(harness, runs)


def test_the_sums_follow_the_stated_order(harness, groups):
    """a vertex's row is, from 0.0, the post-part of segment v - 2, the end-part of v - 1, the start-part of v and the pre-part
    of v + 1, in that order; a path's limit gradients are its segments' parts from 0.0 in increasing index.  Both orders are
    pinned by paths whose sums differ in the last bit when taken in decreasing index."""
    probs = groups["fixture"] + groups["mixed_70"][:24]
    results = bu.run_harness(harness, probs)
    pinned_vertex = pinned_limit = 0
    for p, r in zip(probs, results):
        S = len(p["upstream"])
        if S < 2:
            continue
        parts = _one_hot_contributions(harness, p)
        for k in range(8):
            up = down = 0.0
            for j in range(S):
                up = up + parts[j]["grad_limits"][k]
                down = down + parts[S - 1 - j]["grad_limits"][k]
            assert bu.same_bits(up, r["grad_limits"][k]), k
            pinned_limit += int(not bu.same_bits(up, down))
        for v in range(S + 1):
            segs = [j for j in (v - 2, v - 1, v, v + 1) if 0 <= j < S]
            up, down = np.zeros(4), np.zeros(4)
            for j in segs:
                up = up + parts[j]["grad_waypoints"][v]
            for j in reversed(segs):
                down = down + parts[j]["grad_waypoints"][v]
            assert bu.same_bits(up, r["grad_waypoints"][v]), v
            pinned_vertex += int(len(segs) == 4 and not bu.same_bits(up, down))
            for j in range(S):
                if j not in segs:
                    assert np.all(parts[j]["grad_waypoints"][v] == 0.0)
    assert pinned_vertex >= 1, "no path tells the increasing order of a vertex's four addends from the decreasing one"
    assert pinned_limit >= 1, "no path tells the increasing order of the limit sum from the decreasing one"


def test_zero_upstream_floor_entry_8_and_unusable_segments_give_exact_zeros(harness):
    cases = {c["name"]: c for c in bu.load_cases()}
    c = cases["seven_segments"]
    p = bu.case_problem(c)
    zero = bu.run_harness(harness, [dict(p, upstream=np.zeros_like(p["upstream"]))])[0]
    assert zero["flags"].tolist() == c["flags"]
    assert np.all(bu.bits(zero["grad_waypoints"]) == 0) and np.all(bu.bits(zero["grad_limits"]) == 0)   # +0.0, every entry
    # FLOOR: the 5 mm segment gives nothing; what its neighbours give is theirs alone
    f = bu.case_problem(cases["five_millimetres"])
    full = bu.run_harness(harness, [f])[0]
    without = bu.run_harness(harness, [dict(f, upstream=f["upstream"] * np.array([1.0, 0.0, 1.0]))])[0]
    assert full["flags"][1] & (bu.FLOOR | bu.HEADING) == bu.FLOOR
    assert bu.same_bits(full["grad_waypoints"], without["grad_waypoints"]) and bu.same_bits(full["grad_limits"], without["grad_limits"])
    alone = bu.run_harness(harness, [dict(f, upstream=f["upstream"] * np.array([0.0, 1.0, 0.0]))])[0]
    assert np.all(alone["grad_waypoints"] == 0.0) and np.all(alone["grad_limits"] == 0.0)
    # entry 8 is not read and gets nothing, whatever it holds
    for v in (0.0, 7.5, float("nan")):
        lim = p["limits"].copy()
        lim[8] = v
        r = bu.run_harness(harness, [dict(p, limits=lim)])[0]
        assert r["grad_limits"][8] == 0.0 and r["flags"].tolist() == c["flags"]
        assert bu.same_bits(r["grad_waypoints"], bu.run_harness(harness, [p])[0]["grad_waypoints"])
    # a waypoint that is not a number spoils the segments that read it -- vertex 3's position is read by segments 1 .. 4 -- and
    # only them: FLOOR, zeros; an infinite one the same
    for bad in (float("nan"), float("inf")):
        w = p["waypoints"].copy()
        w[3, 1] = bad
        r = bu.run_harness(harness, [dict(p, waypoints=w)])[0]
        assert r["flags"][1:5].tolist() == [bu.FLOOR] * 4 and r["flags"][[0, 5, 6]].tolist() == [c["flags"][j] for j in (0, 5, 6)]
        only = bu.run_harness(harness, [dict(p, upstream=np.where(np.isin(np.arange(7), (1, 2, 3, 4)), 0.0, p["upstream"]))])[0]
        assert bu.same_bits(r["grad_waypoints"], only["grad_waypoints"]) and bu.same_bits(r["grad_limits"], only["grad_limits"])
    # a heading is read by its own two segments only
    w = p["waypoints"].copy()
    w[3, 3] = float("nan")
    r = bu.run_harness(harness, [dict(p, waypoints=w)])[0]
    assert r["flags"][[2, 3]].tolist() == [bu.FLOOR] * 2 and r["flags"][[0, 1, 4, 5, 6]].tolist() == [c["flags"][j] for j in (0, 1, 4, 5, 6)]
    # a limit that is not a number: every segment of the path
    lim = p["limits"].copy()
    lim[6] = float("nan")
    r = bu.run_harness(harness, [dict(p, limits=lim)])[0]
    assert np.all(r["flags"] == bu.FLOOR) and np.all(r["grad_waypoints"] == 0.0) and np.all(r["grad_limits"] == 0.0)
    # a zero speed limit makes the time infinite: zeros, FLOOR
    lim = p["limits"].copy()
    lim[0] = 0.0
    r = bu.run_harness(harness, [dict(p, limits=lim)])[0]
    assert np.all(np.isfinite(r["grad_waypoints"])) and np.all(np.isfinite(r["grad_limits"]))


def test_translation_changes_nothing(harness, fixture_results):
    """t depends on differences only: every column of a path's waypoint gradient sums to rounding"""
    for c, r in zip(*fixture_results):
        total = np.abs(r["grad_waypoints"].sum(axis=0))
        scale = np.array(c["scale_waypoints"]).sum(axis=0)
        assert np.all(total <= bu.GRAD_RTOL * scale), c["name"]


def _gate_cases():
    t = [1.5, 2.25, 0.75, 3.0]   # total 7.5
    base = dict(seg_times=t, dt=0.2, max_factor=3.0, min_factor=0.33, status=None)
    return [
        (dict(base, n_samples=5), bu.ACCEPTED),                      # 1.0 s: not longer than one second, never checked
        (dict(base, n_samples=4, seg_times=[100.0]), bu.ACCEPTED),   # 0.8 s against 100 s: the same
        (dict(base, n_samples=6, seg_times=[100.0]), bu.TOO_SHORT),  # 1.2 s: checked
        (dict(base, n_samples=38), bu.ACCEPTED),                     # 7.6 s against 7.5
        (dict(base, n_samples=113), bu.TOO_LONG),                    # 22.6 > 22.5
        (dict(base, n_samples=112), bu.ACCEPTED),                    # 22.4
        (dict(base, n_samples=12), bu.TOO_SHORT),                    # 2.4 < 2.475
        (dict(base, n_samples=13), bu.ACCEPTED),                     # 2.6
        (dict(base, n_samples=113, max_factor=0.0), bu.ACCEPTED),    # the long side off
        (dict(base, n_samples=113, max_factor=-1.0), bu.ACCEPTED),
        (dict(base, n_samples=12, min_factor=0.0), bu.ACCEPTED),     # the short side off
        (dict(base, n_samples=12, max_factor=0.0, min_factor=0.0), bu.ACCEPTED),
        (dict(base, n_samples=38, status=1), bu.ACCEPTED),
        (dict(base, n_samples=38, status=5), bu.ACCEPTED),
        (dict(base, n_samples=38, status=-1), bu.ACCEPTED),
        (dict(base, n_samples=38, status=6), bu.REJECTED_CODE),      # MAXTIME
        (dict(base, n_samples=38, status=0), bu.REJECTED_CODE),
        (dict(base, n_samples=38, status=-2), bu.REJECTED_CODE),
        (dict(base, n_samples=113, status=-4), bu.REJECTED_CODE),    # the code comes first
        (dict(base, n_samples=113, status=3), bu.TOO_LONG),
        (dict(base, n_samples=0), bu.ACCEPTED),
    ]


def test_length_gate_is_length_check_and_the_hosts_sum(harness):
    gates = [g for g, _ in _gate_cases()]
    rng = np.random.default_rng(5)
    for _ in range(40):   # sums whose order shows, counts on both sides of both factors
        t = rng.uniform(0.01, 9.0, int(rng.integers(1, 31)))
        total = float(np.sum(t))
        gates.append(dict(seg_times=t, n_samples=int(rng.choice([0.2, 0.9, 1.1, 2.9, 3.1, 5.0]) * total / 0.2), dt=0.2,
                          max_factor=3.0, min_factor=0.33, status=int(rng.choice([1, 4, 6, -1, 0])) if rng.random() < 0.5 else None))
    got = bu.run_gate_harness(harness, gates)
    for n, (g, (total, verdict)) in enumerate(zip(gates, got)):
        want_total, want_verdict = bu.gate_restatement(**g)
        assert bu.same_bits(total, want_total) and verdict == want_verdict, (n, g)
    for (g, want), (_, verdict) in zip(_gate_cases(), got):
        assert verdict == want, g
    assert {v for _, v in got} == {bu.ACCEPTED, bu.REJECTED_CODE, bu.TOO_LONG, bu.TOO_SHORT}
    # the sum's order is observable: some path's total differs from the same sum taken in decreasing index
    assert any(not bu.same_bits(total, bu.gate_restatement(**dict(g, seg_times=np.asarray(g["seg_times"])[::-1]))[0])
               for g, (total, _) in zip(gates, got))


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness, groups):
    san = bu.build_harness(tmp_path, sanitize=True)
    probs = groups["fixture"] + groups["mixed_70"][:12] + groups["uniform_3x1"]
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for a, b in zip(bu.run_harness(san, probs, env=env), bu.run_harness(harness, probs)):
        assert a["raw"] == b["raw"]
    gates = [g for g, _ in _gate_cases()]
    assert bu.run_gate_harness(san, gates, env=env) == bu.run_gate_harness(harness, gates)

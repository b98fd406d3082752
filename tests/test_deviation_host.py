"""The deviation from the waypoint path and its backward pass on the CPU: csrc/mrs_tg_deviation.hpp (the distance, the advance
test and the gradient rows of path_deviation_kernel / path_deviation_vjp_kernel) compiled by g++ into
tests/host/deviation_harness.cpp, against the oracle bit for bit (forward) and against the 60-digit fixtures of
tests/golden/gen_deviation_cases.py (backward).  No GPU."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import deviation_util as du


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return du.build_harness(tmp_path_factory.mktemp("deviation"))


def _fixture_problems():
    out = {}
    for c in du.load_cases():
        g = np.zeros(len(c["samples"]))
        g[:len(c["upstream"])] = c["upstream"]
        out["fixture_" + c["name"]] = du.problem(c["waypoints"], c["samples"], first_segment=c["first_segment"], upstream=g)
    return out


def _all_problems():
    probs = dict(du.small_shapes())
    probs.update(_fixture_problems())
    for q, p in enumerate(du.ragged_batch(12, 5)):
        probs["ragged_%d" % q] = p
    return probs


def test_fixtures_hold_the_required_cases():
    cases = {c["name"]: c for c in du.load_cases()}
    assert {"one_segment", "three_segments", "ten_segments_two_chunks", "cursor_sticks", "starts_behind_w0",
            "tie_exact_coordinates"} <= set(cases)
    assert [n for n, c in cases.items() if c["tie"]] == ["tie_exact_coordinates"]
    assert {b for c in cases.values() if not c["tie"] for b in c["branch"]} == {-1, 0, 1}
    for c in cases.values():
        k = len(c["samples"]) - 1
        assert len(c["cursor"]) == k and len(c["upstream"]) == k and np.array(c["grad_samples"]).shape == (k, 3)
        assert np.array(c["grad_waypoints"]).shape == (len(c["waypoints"]), 3)
        g = np.array(c["upstream"])
        assert np.array_equal(g * 64, np.round(g * 64))   # dyadic
    assert len(cases["one_segment"]["waypoints"]) == 2
    ten = cases["ten_segments_two_chunks"]
    assert max(ten["cursor"]) == 9 and len(ten["cursor"]) > 128
    assert max(cases["cursor_sticks"]["cursor"]) == 0
    tie = cases["tie_exact_coordinates"]
    assert tie["waypoints"][1] == tie["waypoints"][2] and 1 in tie["cursor"] and 0.0 in tie["upstream"]
    assert os.path.getsize(du.FIXTURES) < 64 * 1024


def test_small_shapes_have_the_properties_their_names_state():
    shapes = du.small_shapes()
    scans = {n: du.oracle_scan(po, p) for n, p in shapes.items()}
    moves = {n: (np.nonzero(np.diff(s["cursor"]))[0] + 1).tolist() for n, s in scans.items()}
    for S in (1, 2, 3, 10, 30):
        assert shapes["S%d" % S]["waypoints"].shape[0] == S + 1 and len(moves["S%d" % S]) == S - 1
    for n in (0, 1, 2, 63, 64, 65, 66, 129):
        assert len(scans["n%d" % n]["cursor"]) == max(n - 1, 0)
    assert shapes["overflow"]["n_samples"] == shapes["overflow"]["capacity"] + 1 and len(scans["overflow"]["cursor"]) == 69
    assert moves["seam_63_then_0"] == [64, 65]           # the advances are decided by samples 63 and 64
    assert moves["consecutive_advances"] == [11, 12]
    five = moves["five_advances_in_a_chunk"]
    assert len(five) == 5 and five[-1] < 64
    assert moves["cursor_sticks"] == [] and len(scans["cursor_sticks"]["cursor"]) > 64
    assert scans["cursor_sticks"]["max_deviation"] > 1.0 and scans["cursor_sticks_first_segment_0"]["max_deviation"] == 0.0
    assert scans["cursor_sticks_first_segment_0"]["argmax"] == -1
    w = shapes["coincident_waypoints"]["waypoints"]
    assert np.array_equal(w[2], w[3]) and len(moves["coincident_waypoints"]) == 3
    on = scans["samples_on_their_segment"]["deviation"]
    assert np.sum(on == 0.0) >= 30 and np.sum(on > 0.0) >= 2
    assert scans["first_segment_0"]["max_deviation"] <= scans["first_segment_1"]["max_deviation"]
    assert scans["one_segment_first_segment_0"]["max_deviation"] > 0.0   # n_wp <= 2: counted all the same


def test_forward_is_the_oracles_scan_in_the_same_bits(harness):
    probs = _all_problems()
    res = du.run_harness(harness, list(probs.values()))
    scanned = 0
    for (name, p), r in zip(probs.items(), res):
        o = du.oracle_scan(po, p)
        assert np.array_equal(r["cursor"], o["cursor"]), name
        assert du.same_bits(r["deviation"], o["deviation"]), name
        assert du.same_bits(r["max_deviation"], o["max_deviation"]) and r["argmax"] == o["argmax"], name
        assert du.same_bits(r["segment_max"], o["segment_max"]), name
        scanned += len(o["cursor"])
        for threshold in (0.05, 0.2):
            ok, safe, mx = du.oracle_validate(po, p, threshold)
            v_ok, v_safe, v_mx = r["validate"][threshold]   # devq::validate itself: the policy layer's scan on both routes
            assert v_ok == ok and np.array_equal(v_safe, safe) and du.same_bits(v_mx, mx), (name, threshold)
            assert du.same_bits(r["max_deviation"], mx), (name, threshold)
            assert np.array_equal(r["segment_max"] <= threshold, safe), (name, threshold)
            assert ok == bool(np.all(r["segment_max"] <= threshold)), (name, threshold)
    print("DEVIATION HOST FORWARD: %d problems, %d scanned samples, all bits equal" % (len(probs), scanned))
    assert scanned > 3000


def _bounds(case, deviation):
    """the derived bound of the issue per entry: 16 eps max(|p|, |a|, |b|) / d |g| per contributing sample"""
    w, s, g = np.array(case["waypoints"]), np.array(case["samples"]), np.array(case["upstream"])
    bs, bw = np.zeros((len(g), 3)), np.zeros((len(w), 3))
    for i, c in enumerate(case["cursor"]):
        if deviation[i] == 0.0 or g[i] == 0.0:
            continue   # (contributes exactly 0)
        m = max(np.linalg.norm(s[i]), np.linalg.norm(w[c]), np.linalg.norm(w[c + 1]))
        b = 16.0 * du.EPS * m / deviation[i] * abs(g[i])
        bs[i] += b
        bw[c] += b
        bw[c + 1] += b
    return bs, bw


def test_gradients_match_every_fixture_within_the_derived_bound(harness):
    cases = du.load_cases()
    probs = _fixture_problems()
    res = du.run_harness(harness, [probs["fixture_" + c["name"]] for c in cases])
    report = {}
    for c, r in zip(cases, res):
        assert np.array_equal(r["cursor"], np.array(c["cursor"])), c["name"]
        bs, bw = _bounds(c, r["deviation"])
        es = np.abs(r["grad_samples"] - np.array(c["grad_samples"]))
        ew = np.abs(r["grad_waypoints"] - np.array(c["grad_waypoints"]))
        worst = max(np.max(es / np.maximum(bs, 1e-300) * (es > 0)), np.max(ew / np.maximum(bw, 1e-300) * (ew > 0)))
        report[c["name"]] = "%.1e abs, %.2f of the bound" % (max(es.max(), ew.max()), worst)
        assert np.all(es <= bs), (c["name"], float(np.max(es - bs)))
        assert np.all(ew <= bw), (c["name"], float(np.max(ew - bw)))
    print("DEVIATION HOST GRADIENT FIXTURES: %s" % report)


def test_tie_case_takes_the_forwards_branch_and_exact_zeros(harness):
    c = next(c for c in du.load_cases() if c["tie"])
    r = du.run_harness(harness, [_fixture_problems()["fixture_" + c["name"]]])[0]
    g, d = np.array(c["upstream"]), r["deviation"]
    assert np.sum(d == 0.0) == 2 and np.sum(g == 0.0) == 1
    dead = (d == 0.0) | (g == 0.0)
    assert np.all(r["grad_samples"][dead] == 0.0) and np.all(np.array(c["grad_samples"])[dead] == 0.0)
    # sample 0 sits at coord == 0 and sample 4 at coord == len of segment 0: the interior row, everything perpendicular
    assert r["grad_samples"][0].tolist() == [0.0, 1.0, 0.0] and r["grad_samples"][4].tolist() == [0.0, 1.25, 0.0]
    # sample 5: a segment without length gives everything to its first waypoint
    assert c["cursor"][5] == 1
    lone = du.problem(c["waypoints"], c["samples"], upstream=np.eye(len(c["samples"]))[5])
    rl = du.run_harness(harness, [lone])[0]
    assert np.array_equal(rl["grad_waypoints"][1], -rl["grad_samples"][5]) and np.all(rl["grad_waypoints"][[0, 2, 3]] == 0.0)


def test_status_below_one_and_short_paths_scan_nothing(harness):
    shapes = du.small_shapes()
    dead = dict(shapes["S3"], status=0)
    res = du.run_harness(harness, [dead, shapes["n0"], shapes["n1"]])
    for r in res:
        assert len(r["cursor"]) == 0 and r["max_deviation"] == 0.0 and r["argmax"] == -1
        assert np.all(r["segment_max"] == 0.0) and np.all(r["grad_samples"] == 0.0) and np.all(r["grad_waypoints"] == 0.0)


def test_column_sums_of_the_gradients_cancel(harness):
    """d depends on differences only: moving samples and waypoints together changes nothing, so per sample
    dd/dp + dd/da + dd/db = 0 -- checked with one upstream entry at a time on a path that takes all three branches"""
    p = du.small_shapes()["cursor_sticks"]
    k = du.scanned_rows(p)
    probs = [dict(p, upstream=np.eye(p["capacity"])[i] * 1.5) for i in range(0, k, 7)]
    for i, r in zip(range(0, k, 7), du.run_harness(harness, probs)):
        total = r["grad_samples"][i] + r["grad_waypoints"].sum(axis=0)
        assert np.all(np.abs(total) <= 4 * du.EPS * 1.5), (i, total)
        assert np.all(np.delete(r["grad_samples"], i, axis=0) == 0.0)


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = du.build_harness(tmp_path, sanitize=True)
    probs = list(_all_problems().values())
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for a, b in zip(du.run_harness(san, probs, env=env), du.run_harness(harness, probs)):
        assert a["raw"] == b["raw"]


def test_chain_seeds_keep_every_counted_sample_off_the_path():
    """the paths tests/test_gpu_deviation.py differentiates through solve -> sample -> path_deviation: with the oracle's solve
    and sampler, every counted sample (cursor > 0, first_segment = 0) of the rows that fit has d >= 1e-3, the cursor reaches
    the last segment, and the corridor of 5 cm is left by many of them"""
    batch = du.chain_batch()
    cap = du.CHAIN_CAPACITY
    ref = po.solve_batch(batch.seg_offsets, batch.waypoints, batch.fixed_mask, batch.fixed_values, batch.limits,
                         np.zeros(batch.n_segments), deriv=4, estimate_times=True, sampling_dt=du.CHAIN_DT, sample_capacity=cap)
    assert np.all(ref["status"] > 0) and np.all(ref["n_samples"] > cap)   # (more samples than rows: the scan ends early)
    for p in range(batch.n_paths):
        a, b = batch.seg_offsets[p], batch.seg_offsets[p + 1]
        r = du.oracle_scan_rows(po, batch.waypoints[a + p:b + p + 1], ref["samples"][p], cap - 1, 0)
        counted = r["cursor"] > 0
        assert r["cursor"].max() >= 1 and counted.sum() >= 15, p
        assert r["deviation"][counted].min() >= 1e-3, (p, r["deviation"][counted].min())
        assert np.sum(r["deviation"][counted] > du.CHAIN_CORRIDOR) >= 10, p

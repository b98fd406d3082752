"""The waypoint passage and its backward pass on the CPU: csrc/mrs_tg_passage.hpp (the distance, the foot point, the gradient
rows and the reference loops that waypoint_passage_kernel / waypoint_passage_vjp_kernel are held to) compiled by g++ into
tests/host/passage_harness.cpp, against the oracle bit for bit (forward) and against the 60-digit fixtures of
tests/golden/gen_passage_cases.py (backward).  No GPU."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import deviation_util as du
from tests import passage_util as pu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return pu.build_harness(tmp_path_factory.mktemp("passage"))


def _fixture_problems():
    return {"fixture_" + c["name"]: pu.problem(c["waypoints"], c["samples"], grad_miss=c["grad_miss"],
                                               grad_fraction=c["grad_fraction"]) for c in pu.load_cases()}


def _all_problems():
    probs = dict(pu.small_shapes())
    probs.update(_fixture_problems())
    for every, extra in ((1, 0), (2, 0), (1, 3)):
        for q, p in enumerate(pu.ragged_batch(8, 5, every=every, extra=extra)[0]):
            probs["ragged_%d_%d_%d" % (every, extra, q)] = p
    return probs


def test_fixtures_hold_the_required_cases():
    cases = {c["name"]: c for c in pu.load_cases()}
    assert {b for c in cases.values() for b in c["branch"]} == {-1, 0, 1}
    assert cases["across_the_seam"]["index"][-2:] == [63, 64]
    for c in cases.values():
        w, s = np.array(c["waypoints"]), np.array(c["samples"])
        assert len(c["index"]) == len(w) == len(c["grad_miss"]) == len(c["grad_fraction"])
        for tag in ("miss", "fraction"):
            assert np.array(c["grad_samples_" + tag]).shape == s.shape and np.array(c["grad_waypoints_" + tag]).shape == w.shape
        g = np.array(c["grad_miss"] + c["grad_fraction"])
        assert np.array_equal(g * 64, np.round(g * 64)) and np.all(g != 0)   # dyadic
        for k, i in enumerate(c["index"]):   # the margins the issue asks for: the bounds mean something
            assert np.linalg.norm(s[i + 1] - s[i]) >= 0.05 and pu.oracle_dist(po, w[k], s[i], s[i + 1]) >= 1e-4
    assert max(np.abs(np.array(cases["far_from_the_origin"]["samples"])).max(), 1) >= 40
    assert os.path.getsize(pu.FIXTURES) < 64 * 1024


def test_small_shapes_have_the_properties_their_names_state():
    shapes = pu.small_shapes()
    scans = {n: pu.oracle_scan(po, p) for n, p in shapes.items()}
    idx = {n: s["index"][:s["count"]].tolist() for n, s in scans.items()}
    for W in (1, 2, 5, 31):
        assert len(shapes["W%d" % W]["waypoints"]) == W and scans["W%d" % W]["count"] == W
    for n in (0, 1, 2, 63, 64, 65, 66, 129):
        p = shapes["n%d" % n]
        assert pu.rows(p) == n and (scans["n%d" % n]["count"] >= 1) == (n >= 2)
    assert shapes["overflow"]["n_samples"] == shapes["overflow"]["capacity"] + 1 == 71
    assert idx["hit_on_lane_63"] == [63, 90] and idx["hit_on_lane_0_of_chunk_2"] == [20, 64]
    assert idx["hits_on_steps_63_and_64"] == [10, 63, 64, 100]
    assert idx["hit_on_the_last_step_of_a_full_chunk"] == [5, 63] and pu.rows(shapes["hit_on_the_last_step_of_a_full_chunk"]) == 65
    assert idx["adjacent_steps"] == [11, 12, 30]
    assert len(idx["five_hits_in_a_chunk"]) == 5 and idx["five_hits_in_a_chunk"][-1] < 64
    assert idx["seventy_collinear"] == list(range(70))
    never = shapes["never_reached_with_near_ones_behind"]
    assert idx["never_reached_with_near_ones_behind"] == [5] and scans["never_reached_with_near_ones_behind"]["index"].tolist() == [5, -1, -1, -1]
    assert pu.oracle_scan(po, dict(never, waypoints=never["waypoints"][2:]))["count"] == 2   # (the ones behind it ARE near)
    back = shapes["all_reached_early_then_back_at_w0"]
    assert idx["all_reached_early_then_back_at_w0"] == [3, 10]
    assert pu.oracle_scan(po, dict(back, samples=back["samples"][40:], n_samples=40))["count"] >= 1   # it does come back
    assert idx["nan_row_passed_over"] == [10, 50] and idx["nan_row_blocks"] == [10]
    assert np.isnan(shapes["nan_row_blocks"]["samples"][30, 1])
    co = shapes["coincident_samples"]
    assert idx["coincident_samples"] == [19, 20, 41] and np.array_equal(co["samples"][20], co["samples"][21])
    on = scans["waypoint_on_its_step"]
    assert on["index"].tolist() == [4, 9, 20] and on["miss"].tolist() == [0.0, 0.0, 0.0625]
    assert len(shapes["no_waypoints"]["waypoints"]) == 0 and scans["no_waypoints"]["count"] == 0
    assert scans["threshold_at_0p1_is_no_hit"]["count"] == 0 and scans["threshold_below_0p1_is_a_hit"]["count"] == 1


def test_forward_is_the_oracles_scan_in_the_same_bits(harness):
    """index, count and miss of the harness are mto_waypoint_trajectory_idxs / mto_dist_from_segment on every fixture, small
    shape and ragged path; where the library loads, index and count are the host's mrs_tg_waypoint_trajectory_idxs as well"""
    probs = _all_problems()
    res = pu.run_harness(harness, list(probs.values()))
    try:
        from mrs_uav_trajectory_generation_amd import api
        api.load_library()
    except Exception:   # (a machine without the built library still runs the oracle's comparison)
        api = None
    reached = wanted = with_host = 0
    for (name, p), r in zip(probs.items(), res):
        o = pu.oracle_scan(po, p)
        assert r["count"] == o["count"] and np.array_equal(r["index"], o["index"]), name
        assert pu.same_bits(r["miss"], o["miss"]), name
        k = r["count"]
        assert np.all(r["fraction"][k:] == 0.0) and np.all((r["fraction"][:k] >= 0.0) & (r["fraction"][:k] <= 1.0)), name
        assert np.all(np.diff(r["index"][:k]) > 0), name
        reached += k
        wanted += len(p["waypoints"])
        m = pu.rows(p) if p["status"] > 0 else 0
        if api is not None and m >= 2 and len(p["waypoints"]) > 0:
            host = api.waypoint_trajectory_idxs(pu._pad4(p["samples"][:m]), pu._pad4(p["waypoints"]))
            assert host.tolist() == r["index"][:k].tolist(), name
            with_host += 1
    print("PASSAGE HOST FORWARD: %d problems (%d against the library's host scan), %d of %d waypoints reached, all bits equal" %
          (len(probs), with_host, reached, wanted))
    assert reached > 400 and reached < wanted


def test_library_host_scan_at_its_empty_and_last_step_edges():
    """mrs_tg_waypoint_trajectory_idxs (the policy layer's host scan, written with passq::hit) against
    mto_waypoint_trajectory_idxs: no waypoint (0, and nothing read), one waypoint with 0, 1 and 2 samples, and a path whose last
    waypoint is taken by the last step.  Entries behind the count are left alone.  Needs the built library (build() of
    __graft_entry__.py), as the GPU tests do, and no GPU: without it this test fails rather than skips, since the function under
    test exists nowhere else."""
    import ctypes as C
    from mrs_uav_trajectory_generation_amd import api
    L = api.load_library()

    def host(samples3, n, waypoints3):
        smp = pu._pad4(np.asarray(samples3, dtype=np.float64).reshape(-1, 3))
        wps = pu._pad4(np.asarray(waypoints3, dtype=np.float64).reshape(-1, 3))
        arr, _ = api._waypoint_array([wps if len(wps) else np.zeros((1, 4))])
        idx = np.full(len(wps) + 4, -7, dtype=np.int32)
        k = L.mrs_tg_waypoint_trajectory_idxs(api._np_ptr(smp if len(smp) else np.zeros((1, 4))), n,
                                              arr.ctypes.data_as(C.POINTER(api.Waypoint)), len(wps), api._np_ptr(idx))
        assert np.all(idx[k:] == -7)
        return k, idx[:k].tolist(), smp, wps

    walk = pu.straight(12)
    assert host(walk, 12, np.zeros((0, 3)))[:2] == (0, [])          # W = 0: nothing to pass (the waypoint array is not read)
    one = [[0.3, 0.3, 0.0]]
    last = [[0.3, 0.3, 0.0], [1.3, 0.32, 0.0], [pu.STEP * 10.5, 0.3, 0.02]]   # w_2 sits on the step 10 -> 11, the last one
    for n, wps in ((0, one), (1, one), (2, one), (12, one), (12, last), (11, last)):
        k, idx, smp, w4 = host(walk[:max(n, 0)], n, wps)
        o = pu.oracle_scan_rows(po, w4, smp if n else np.zeros((1, 4)), n)
        assert k == o["count"] and idx == o["index"][:k].tolist(), (n, len(wps))
        if (n, len(wps)) in ((0, 1), (1, 1), (12, 3), (11, 3)):
            assert k == {(0, 1): 0, (1, 1): 0, (12, 3): 3, (11, 3): 2}[(n, len(wps))], (n, len(wps), k)
    assert host(walk, 12, last)[1][-1] == 10


def _one(p, a, b, **kw):
    return pu.problem([p], [a, b], **kw)


def test_fraction_is_its_closed_form_on_exactly_representable_cases(harness):
    a, b = [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]
    cases = [([0.0, 0.0625, 0.0], 0.0, 0.0625),      # coord == 0: the interior row
             ([0.5, 0.0625, 0.0], 1.0, 0.0625),      # coord == len: the interior row
             ([0.25, 0.0625, 0.0], 0.5, 0.0625),     # the foot point in the middle
             ([0.375, 0.0, -0.03125], 0.75, 0.03125),
             ([-0.0625, 0.0, 0.0], 0.0, 0.0625),     # in front of the start
             ([0.5625, 0.0, 0.0], 1.0, 0.0625)]      # behind the end
    probs = [_one(p, a, b) for p, _, _ in cases] + [_one([0.0, 0.0625, 0.0], a, a)]   # len == 0
    res = pu.run_harness(harness, probs)
    for (p, tau, m), r in zip(cases + [(None, 0.0, 0.0625)], res):
        assert r["count"] == 1 and r["index"].tolist() == [0], p
        assert r["fraction"].tolist() == [tau] and r["miss"].tolist() == [m], (p, r["fraction"], r["miss"])


def test_kinks_take_the_forwards_branch_and_exact_zeros(harness):
    """coord == 0 and coord == len take the interior row of the fraction; the clamped branches and len == 0 give it exactly 0;
    m == 0 gives exactly 0 through the miss; a zero upstream gives exactly 0"""
    a, b = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]
    f = dict(grad_miss=[0.0], grad_fraction=[1.0])
    at0, at_len, front, behind, flat, on, dead = pu.run_harness(harness, [
        _one([0.0, 0.0625, 0.0], a, b, **f), _one([1.0, 0.0625, 0.0], a, b, **f), _one([-0.0625, 0.0, 0.0], a, b, **f),
        _one([1.0625, 0.0, 0.0], a, b, **f), _one([0.0, 0.0625, 0.0], a, a, **f),
        _one([0.25, 0.0, 0.0], a, b, grad_miss=[1.5], grad_fraction=[0.0]),
        _one([0.25, 0.0625, 0.0], a, b, grad_miss=[0.0], grad_fraction=[0.0])])
    # v = (1, 0, 0), L2 = 1: dtau/dp = v, dtau/db = q - 2 tau v, dtau/da = -dtau/dp - dtau/db
    assert at0["grad_waypoints"].tolist() == [[1.0, 0.0, 0.0]]
    assert at0["grad_samples"].tolist() == [[-1.0, -0.0625, 0.0], [0.0, 0.0625, 0.0]]
    assert at_len["grad_waypoints"].tolist() == [[1.0, 0.0, 0.0]]
    assert at_len["grad_samples"].tolist() == [[0.0, -0.0625, 0.0], [-1.0, 0.0625, 0.0]]
    for r in (front, behind, flat, on, dead):
        assert r["count"] == 1 and np.all(r["grad_waypoints"] == 0.0) and np.all(r["grad_samples"] == 0.0)
    assert on["miss"].tolist() == [0.0]


def _hits(c):
    w, s = np.array(c["waypoints"]), np.array(c["samples"])
    return [(k, i, w[k], s[i], s[i + 1]) for k, i in enumerate(c["index"])]


def test_gradients_match_every_fixture_within_the_derived_bounds(harness):
    """The harness's rows against 60-digit central differences, the indices held fixed, the two upstreams one at a time.

    Miss rows: the bound the project derived for devq::dist_vjp, 16 eps max(|p|, |a|, |b|) / m |g| per entry and hit.

    Fraction rows: the first-order rounding bound of the operation sequence csrc/mrs_tg_passage.hpp writes down, with
    u = eps / 2 the unit roundoff, v = b - a, q = p - a, len = |v|, the inputs exact doubles:
      v_k, q_k            one subtraction of two inputs each: relative error u (so no |p| / len factor arises: nothing of the
                          inputs' own magnitude is ever rounded, unlike the foot point a + n coord of the distance)
      len                 three squares, two additions, a root: relative 4 u;   L2 = len len: 9 u;   n_k = v_k / len: 6 u
      coord = sum n_k q_k products 8 u, two additions 2 u, on sum |n_k q_k| <= |q|: absolute 10 u |q|
      tau = coord / len   (10 u |q| + 4 u coord) / len + u tau <= 15 u |q| / len   (tau <= |q| / len);   t2 = 2 tau is exact
      tp_k = v_k / L2     relative 11 u: absolute 11 u / len
      tb_k                t2 v_k: 2 |v_k| (15 + 2) u |q| / len <= 34 u |q|;  q_k: u |q|;  the difference, at most 3 |q| large:
                          3 u |q|;  the division by L2: 38 u |q| / L2 + 10 u 3 |q| / L2 = 68 u |q| / L2
      ta_k                11 u / len + 68 u |q| / L2 + u (1 / len + 3 |q| / L2) = 12 u / len + 71 u |q| / L2
      times g             one more u of the value: at most (13 / len + 74 |q| / L2) u |g| = (6.5 / len + 37 |q| / L2) eps |g|
    and the fixture's own rounding to a double, u of the value.  Asserted: 40 eps (1 + |q| / len) / len |g| per entry and hit.
    Measured shares of the two bounds are printed (DESIGN.md section 11c records them)."""
    cases = pu.load_cases()
    share = dict(miss=0.0, fraction=0.0)
    for tag, other in (("miss", "grad_fraction"), ("fraction", "grad_miss")):
        probs = [pu.problem(c["waypoints"], c["samples"], **{"grad_" + tag: c["grad_" + tag], other: np.zeros(len(c["index"]))})
                 for c in cases]
        for c, r in zip(cases, pu.run_harness(harness, probs)):
            assert r["index"].tolist() == c["index"], c["name"]
            bs, bw = np.zeros((len(c["samples"]), 3)), np.zeros((len(c["waypoints"]), 3))
            for k, i, p, a, b in _hits(c):
                g = c["grad_" + tag][k]
                bound = pu.miss_bound(p, a, b, r["miss"][k], g) if tag == "miss" else \
                    (pu.fraction_bound(p, a, b, g) if c["branch"][k] == 0 else 0.0)
                bw[k] += bound
                bs[i] += bound
                bs[i + 1] += bound
            es = np.abs(r["grad_samples"] - np.array(c["grad_samples_" + tag]))
            ew = np.abs(r["grad_waypoints"] - np.array(c["grad_waypoints_" + tag]))
            assert np.all(es <= bs), (tag, c["name"], float(np.max(es - bs)))
            assert np.all(ew <= bw), (tag, c["name"], float(np.max(ew - bw)))
            for e, bnd in ((es, bs), (ew, bw)):
                share[tag] = max(share[tag], float(np.max(e[bnd > 0] / bnd[bnd > 0], initial=0.0)))
            if tag == "fraction":   # the clamped branches give exact zeros, in the fixture as in the harness
                for k, i, *_ in _hits(c):
                    if c["branch"][k] != 0:
                        assert np.all(r["grad_waypoints"][k] == 0.0) and np.all(np.array(c["grad_waypoints_fraction"])[k] == 0.0)
    print("PASSAGE HOST GRADIENT FIXTURES: largest share of the miss bound %.3f, of the fraction bound %.3f" %
          (share["miss"], share["fraction"]))


def test_the_two_parts_are_summed_in_the_stated_order(harness):
    """a hit's contribution is accumulate(miss part, fraction part) per coordinate; a waypoint's row is that one term, so the
    run with both upstreams is the rounded sum of the two runs with one; sample row j is 0.0, then the b-part of the hit on
    step j - 1, then the a-part of the hit on step j (rows 12 and 64 of these shapes take both).  Compared as values: a part
    that is exactly zero may carry either sign."""
    shapes = pu.small_shapes()
    for name, row in (("adjacent_steps", 12), ("hits_on_steps_63_and_64", 64)):
        p = shapes[name]
        zero = np.zeros(len(p["waypoints"]))
        both, m_only, t_only = pu.run_harness(harness, [p, dict(p, grad_fraction=zero), dict(p, grad_miss=zero)])
        assert np.array_equal(both["grad_waypoints"], m_only["grad_waypoints"] + t_only["grad_waypoints"]), name
        assert np.all((m_only["grad_waypoints"] != 0).any(axis=1) & (t_only["grad_waypoints"] != 0).any(axis=1)), name
        k = both["index"].tolist().index(row)
        singles = []
        for kk in (k - 1, k):   # the hit on step row - 1 alone (its b-part lands on `row`), the hit on step row alone
            one = np.zeros(len(zero))
            one[kk] = 1.0
            singles.append(pu.run_harness(harness, [dict(p, grad_miss=p["grad_miss"] * one, grad_fraction=p["grad_fraction"] * one)])[0])
        want = (0.0 + singles[0]["grad_samples"][row]) + singles[1]["grad_samples"][row]
        assert np.array_equal(both["grad_samples"][row], want), name
        assert np.any(singles[0]["grad_samples"][row] != 0.0) and np.any(singles[1]["grad_samples"][row] != 0.0), name


def test_the_threshold_is_strict_in_the_bits_of_the_distance(harness):
    """a waypoint whose distance, as dist computes it, is the double nearest 0.1 or above is no hit; the next double below
    is a hit.  Axis-parallel: D = |y| in bits.  Oblique: the offset along a direction is bisected over the doubles until two
    neighbouring offsets have D on the two sides of 0.1 (D is the oracle's, which the harness equals in bits)."""
    tenth = 0.1
    a, b = np.array([0.3, -1.7, 2.2]), np.array([0.9, -1.1, 2.5])
    side = np.cross(b - a, [0.1, 0.7, -0.2])
    side /= np.linalg.norm(side)
    mid = a + 0.4 * (b - a)
    D = lambda t: pu.oracle_dist(po, mid + t * side, a, b)   # noqa: E731
    lo, hi = 0.09, 0.11
    assert D(lo) < tenth <= D(hi)
    while np.nextafter(lo, 1.0) < hi:
        t = 0.5 * (lo + hi)
        lo, hi = (t, hi) if D(t) < tenth else (lo, t)
    assert D(lo) < tenth <= D(hi) and hi == np.nextafter(lo, 1.0)
    below = float(np.nextafter(tenth, 0.0))
    probs = [_one([0.5, tenth, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]), _one([0.5, below, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]),
             _one(mid + hi * side, a, b), _one(mid + lo * side, a, b)]
    assert pu.oracle_dist(po, probs[0]["waypoints"][0], [0, 0, 0], [1, 0, 0]) == tenth
    res = pu.run_harness(harness, probs)
    assert [r["count"] for r in res] == [0, 1, 0, 1]
    assert res[1]["miss"].tolist() == [below] and pu.same_bits(res[3]["miss"], [D(lo)])
    assert res[0]["index"].tolist() == [-1] and res[0]["miss"].tolist() == [0.0] and res[0]["fraction"].tolist() == [0.0]
    print("PASSAGE HOST THRESHOLD: oblique offsets %r (D %r, a hit) and %r (D %r, none)" % (lo, D(lo), hi, D(hi)))


def test_status_below_one_and_short_paths_reach_nothing(harness):
    shapes = pu.small_shapes()
    dead = dict(shapes["W5"], status=0)
    for r in pu.run_harness(harness, [dead, shapes["n0"], shapes["n1"], shapes["no_waypoints"]]):
        assert r["count"] == 0 and np.all(r["index"] == -1) and np.all(r["miss"] == 0.0) and np.all(r["fraction"] == 0.0)
        assert np.all(r["grad_samples"] == 0.0) and np.all(r["grad_waypoints"] == 0.0)


def test_unreached_upstreams_are_never_used(harness):
    p = pu.small_shapes()["never_reached_with_near_ones_behind"]
    nan = np.array([1.0, np.nan, np.nan, np.nan])
    r, q = pu.run_harness(harness, [dict(p, grad_miss=p["grad_miss"] * nan, grad_fraction=p["grad_fraction"] * nan), p])
    assert r["raw"] == q["raw"] and np.all(r["grad_waypoints"][1:] == 0.0)


def test_column_sums_of_the_gradients_cancel(harness):
    """m and tau depend on differences only: moving the waypoint and the two samples together changes nothing"""
    p = pu.small_shapes()["W31"]
    r = pu.run_harness(harness, [p])[0]
    total = r["grad_samples"].sum(axis=0) + r["grad_waypoints"].sum(axis=0)
    scale = np.abs(r["grad_samples"]).sum() + np.abs(r["grad_waypoints"]).sum()
    assert r["count"] == 31 and np.all(np.abs(total) <= 64 * pu.EPS * scale), (total, scale)


def test_harness_under_address_and_undefined_behaviour_sanitizers(tmp_path, harness):
    san = pu.build_harness(tmp_path, sanitize=True)
    probs = list(_all_problems().values())
    env = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for a, b in zip(pu.run_harness(san, probs, env=env), pu.run_harness(harness, probs)):
        assert a["raw"] == b["raw"]


def test_chain_paths_keep_every_hit_off_the_trajectory():
    """the paths tests/test_gpu_passage.py differentiates through solve -> sample -> waypoint_passage: with the oracle's solve
    and sampler and the requested waypoints of pu.chain_request (the vertices moved off the path), every path reaches all five
    waypoints within its rows and every hit has m >= 1e-3, so that the relative stage bound of the miss rows,
    16 eps max(|p|, |a|, |b|) / m, stays below 1e-11; at least two hits per path are interior ones on steps of 0.05 or more,
    so the fraction has a gradient.  (A trajectory that starts at rest has a first step of some 1e-5: the waypoint it takes lies
    far in front of or behind such a step, in a clamped branch, where the fraction has no gradient.)"""
    batch = du.chain_batch()
    cap = pu.CHAIN_CAPACITY
    ref = po.solve_batch(batch.seg_offsets, batch.waypoints, batch.fixed_mask, batch.fixed_values, batch.limits,
                         np.zeros(batch.n_segments), deriv=4, estimate_times=True, sampling_dt=du.CHAIN_DT, sample_capacity=cap)
    assert np.all(ref["status"] > 0) and np.all(ref["n_samples"] < cap)
    req = pu.chain_request(batch)
    for p in range(batch.n_paths):
        n = int(ref["n_samples"][p])
        r = pu.oracle_scan_rows(po, req[5 * p:5 * p + 5], ref["samples"][p], n)
        assert r["count"] == 5, (p, r)
        interior = 0
        for k in range(5):
            i = r["index"][k]
            w, a, b = req[5 * p + k, :3], ref["samples"][p][i, :3], ref["samples"][p][i + 1, :3]
            assert r["miss"][k] >= 1e-3 and pu.miss_bound(w, a, b, r["miss"][k], 1.0) < 1e-11, (p, k)
            ln = np.linalg.norm(b - a)
            coord = np.dot(w - a, b - a) / ln
            assert ln > 0.0 and min(abs(coord), abs(coord - ln)) > 1e-4, (p, k, coord, ln)   # (no hit sits on a kink)
            interior += int(0 < coord < ln and ln >= 0.05)
        assert interior >= 2, (p, interior)

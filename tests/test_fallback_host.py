"""csrc/mrs_tg_fallback.hpp on the CPU (tests/host/fallback_harness.cpp, plain g++ and once more under ASan + UBSan): the whole
findTrajectoryFallback against the oracle's mto_fallback_sampling bit for bit (the same libm on the same machine), the heading
unwrap against the oracle's, the explicit-time edge cases against a restatement of the reference's loop as written, and the
backward sums against a restatement in Python floats in the pinned order.  NaN and inf are ordinary data here."""
import math

import numpy as np
import pytest

from tests import fallback_util as fu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fu.build_harness(tmp_path_factory.mktemp("fallback_host"))


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    return fu.build_harness(tmp_path_factory.mktemp("fallback_host_san"), sanitize=True)


@pytest.fixture(scope="module")
def batches():
    return fu.shapes()


def _with_upstream(p, seed, poison=True):
    """the problem with a dyadic upstream; rows at and beyond min(count, capacity) hold NaN: never read"""
    ref = fu.reference_loop(p)
    n = min(ref["count"], p["capacity"])
    rng = np.random.default_rng(seed)
    up = fu.bu.dyadic(rng, p["capacity"] * 4).reshape(p["capacity"], 4)
    if poison:
        up[n:] = np.nan
    return dict(p, upstream=up), ref


@pytest.mark.parametrize("shape", ["uniform_3x1", "uniform_70x3", "mixed_70", "one_path"])
def test_full_chain_is_the_oracle_in_bits(harness, batches, shape):
    chains = fu.chains(batches[shape], 50)
    chains += [dict(c, relax=not c["relax"]) for c in chains]      # every path with a relaxed and with an unrelaxed heading
    got = fu.run_chain_harness(harness, chains)
    rows = stops = relaxed = 0
    for q, (c, g) in enumerate(zip(chains, got)):
        assert fu.same_bits(g["unwrapped"], fu.oracle_unwrap(c["waypoints"])), q
        unwrapped = np.array(c["waypoints"])
        unwrapped[:, 3] = g["unwrapped"]
        n, ref = fu.oracle_chain(c)
        assert g["count"] == n and n <= c["capacity"], (q, g["count"], n)
        assert fu.same_bits(g["rows"], ref), q       # x, y, z and the heading
        rows, stops, relaxed = rows + n, stops + int(c["stop_at"][1:-1].sum()), relaxed + int(c["relax"])
    assert rows > 0 and relaxed == len(chains) // 2 and (shape == "uniform_3x1" or stops > 0)


def test_unwrap_moves_headings_and_copies_nothing_else(harness, batches):
    chains = fu.chains(batches["mixed_70"], 50)
    got = fu.run_chain_harness(harness, chains)
    moved = sum(int(np.sum(g["unwrapped"] != c["waypoints"][:, 3])) for c, g in zip(chains, got))
    assert moved > 100
    for c, g in zip(chains, got):
        assert g["unwrapped"][0] == c["waypoints"][0, 3]
        assert np.all(np.abs(np.diff(g["unwrapped"])) <= math.pi)


def _check_against_reference(p, h, ref):
    name = p["name"]
    assert h["n_samples"] == ref["n_samples"], (name, h["n_samples"], ref["n_samples"])
    if ref["count"] <= p["capacity"]:
        assert h["count"] == ref["count"], name
    else:
        assert h["count"] > p["capacity"], name
    assert np.array_equal(h["seg_first_row"], ref["seg_first_row"]), (name, h["seg_first_row"], ref["seg_first_row"])
    assert fu.same_bits(h["rows"], ref["rows"]), name


@pytest.fixture(scope="module")
def edge():
    return fu.edge_cases()


def test_edge_cases_are_the_reference_loop_in_bits(harness, edge):
    got = fu.run_harness(harness, edge)
    by_name = {}
    for p, h in zip(edge, got):
        ref = fu.reference_loop(p)
        _check_against_reference(p, h, ref)
        by_name[p["name"]] = (p, h)
    # the cases are what their names say
    assert by_name["t exactly 0.1 gives no rows"][1]["seg_first_row"].tolist() == [0, 4, 4]
    assert by_name["t one ulp above 0.1"][1]["seg_first_row"].tolist() == [0, 4, 5]
    assert by_name["t / dt an exact integer"][1]["count"] == 4 + 6 + 1
    assert by_name["t / dt one ulp above an integer"][1]["count"] == 5 + 7 + 1
    p, h = by_name["negative, NaN and +inf times"]
    assert h["seg_first_row"].tolist() == [0, 0, 0, 5] and h["n_samples"] == 51 and h["rows"].shape[0] == 50
    assert np.all(h["rows"][5:, :3] == p["waypoints"][3, :3])         # step 1 / inf: every row of the segment is its start
    assert by_name["+inf in front, the rest saturated"][1]["seg_first_row"].tolist() == [0, 21, 21]
    assert by_name["every segment at most 0.1"][1]["count"] == 0
    p, h = by_name["a last segment without rows"]
    assert h["count"] == 10 and not np.any(np.all(h["rows"][:, :3] == p["waypoints"][3, :3], axis=1))
    assert by_name["one segment"][1]["count"] == 8 and by_name["one segment without rows"][1]["count"] == 0
    assert by_name["stop_at at vertex 0 and at the last vertex"][1]["count"] == 16
    assert by_name["stop_at at a vertex whose segment has no rows"][1]["count"] == 11
    assert by_name["stop_at in the middle"][1]["count"] == 36
    assert by_name["insert 0 (stopping_time / dt = 0.4)"][1]["count"] == 16
    assert by_name["insert 3 (stopping_time / dt = 2.5)"][1]["count"] == 22
    assert by_name["capacity equal to the count"][1]["n_samples"] == 36
    assert by_name["capacity one below the count"][1]["n_samples"] == 36 and by_name["capacity one below the count"][1]["rows"].shape[0] == 35
    p, h = by_name["capacity inside a dwell"]
    assert h["n_samples"] == 10 and fu.same_bits(h["rows"][5:9], np.tile(h["rows"][5], (4, 1)))
    assert by_name["capacity 1"][1]["rows"].shape[0] == 1
    p, h = by_name["a == b with t > 0.1"]
    assert fu.same_bits(h["rows"][5:10, :3], np.tile(p["waypoints"][1, :3], (5, 1)))
    p, h = by_name["an interpolated yaw next to pi"]
    assert np.all(math.pi - np.abs(h["rows"][:, 3]) < 3e-12)
    p, h = by_name["a heading difference of exactly pi"]
    assert np.all(np.isfinite(h["rows"]))
    assert by_name["a path of 65 segments"][1]["seg_first_row"][64] > 64
    p, h = by_name["rows straddle 63 | 64"]
    assert h["seg_first_row"][12] == 60 and h["seg_first_row"][13] == 68
    p, h = by_name["a dwell straddles 63 | 64"]
    assert h["seg_first_row"][12] == 60 and h["seg_first_row"][13] == 75 and fu.same_bits(h["rows"][60:71], np.tile(h["rows"][60], (11, 1)))


def test_refused_arguments(harness):
    w, t = fu._line(2), [0.9, 0.9]
    bad = [fu.problem(w, t, 0.0, 10), fu.problem(w, t, -0.2, 10), fu.problem(w, t, float("nan"), 10),
           fu.problem(w, t, float("inf"), 10), fu.problem(w, t, 0.2, 10, stopping_time=-1.0),
           fu.problem(w, t, 0.2, 10, stopping_time=float("inf")), fu.problem(w, t, 1e-12, 10, stopping_time=1.0),
           fu.problem(w, t, 0.2, 0), fu.problem(w, t, 0.2, 2 ** 31 - 1)]     # capacity + 1 would not fit int32
    assert fu.run_harness(harness, bad) == [None] * len(bad)
    ok = fu.run_harness(harness, [fu.problem(w, t, 0.2, 10, stopping_time=0.0)])
    assert ok[0] is not None and ok[0]["count"] == 11


def test_backward_is_the_restatement_in_bits(harness, edge, batches):
    probs, refs = [], []
    for n, p in enumerate(edge + fu.batch_problems(batches["mixed_70"], 60)[:20] + fu.batch_problems(batches["one_path"], 61)):
        q, ref = _with_upstream(p, 700 + n)
        probs.append(q), refs.append(ref)
    got = fu.run_harness(harness, probs)
    nonzero = 0
    for p, h, ref in zip(probs, got, refs):
        assert np.isnan(p["upstream"][min(ref["count"], p["capacity"]):]).all()
        want = fu.backward_restatement(p, ref)
        assert np.all(np.isfinite(h["grad_waypoints"])), p["name"]   # the NaN rows were never read
        assert fu.same_bits(h["grad_waypoints"], want), p["name"]
        nonzero += int(np.count_nonzero(want))
    assert nonzero > 1000


def test_a_zero_upstream_gives_exact_zeros(harness, edge):
    probs = [dict(p, upstream=np.zeros((p["capacity"], 4))) for p in edge]
    probs += [dict(p, upstream=-np.zeros((p["capacity"], 4))) for p in edge[:4]]
    for p, h in zip(probs, fu.run_harness(harness, probs)):
        assert fu.same_bits(h["grad_waypoints"], np.zeros_like(h["grad_waypoints"])), p["name"]


def test_the_order_of_the_sums_is_pinned(harness):
    """S = 1, t = 0.6, dt = 0.2: four rows with coeff 0, 1/3, 2/3, 1.  Column 0 of the upstream is chosen so that the second
    vertex's addends are 0, 2^-53, 2^-53, 1.0: increasing row index gives ((0 + 2^-53) + 2^-53) + 1.0 = 1 + 2^-52, decreasing
    gives ((1.0 + 2^-53) + 2^-53) + 0 = 1.0 (each half-ulp addend is lost to the tie).  The harness must give the first."""
    w = fu._line(1)
    p = fu.problem(w, [0.6], 0.2, 8)
    ref = fu.reference_loop(p)
    assert ref["count"] == 4 and ref["row_segment"] == [0, 0, 0, 0]
    c = ref["row_coeff"]
    assert c[0] == 0.0 and c[3] == 1.0
    h = 2.0 ** -53
    up = np.zeros((8, 4))
    up[1, 0], up[2, 0], up[3, 0] = h / c[1], h / c[2], 1.0
    for tries in range(64):   # make the two small addends exactly 2^-53 after the rounding of coeff * g
        if c[1] * up[1, 0] == h and c[2] * up[2, 0] == h:
            break
        for r in (1, 2):
            if c[r] * up[r, 0] < h:
                up[r, 0] = math.nextafter(up[r, 0], 1.0)
            elif c[r] * up[r, 0] > h:
                up[r, 0] = math.nextafter(up[r, 0], 0.0)
    assert c[1] * up[1, 0] == h and c[2] * up[2, 0] == h
    up[4:] = np.nan
    p = dict(p, upstream=up)
    forward = fu.backward_restatement(p, ref)
    backward = fu.backward_restatement(p, ref, reverse=True)
    assert forward[1, 0] == 1.0 + 2.0 ** -52 and backward[1, 0] == 1.0
    assert not fu.same_bits(forward, backward)
    got = fu.run_harness(harness, [p])[0]
    assert fu.same_bits(got["grad_waypoints"], forward)


def test_everything_once_more_under_the_sanitizers(harness, harness_san, edge, batches):
    """the stand-alone harness built with ASan + UBSan gives the plain build's lines on the chains, the edge cases and the
    backward pass"""
    chains = fu.chains(batches["mixed_70"], 50)[:25] + fu.chains(batches["one_path"], 51)
    for a, b in zip(fu.run_chain_harness(harness, chains), fu.run_chain_harness(harness_san, chains)):
        assert a["count"] == b["count"] and fu.same_bits(a["rows"], b["rows"]) and fu.same_bits(a["seg_times"], b["seg_times"])
    probs = [_with_upstream(p, 900 + n)[0] for n, p in enumerate(edge)]
    for p, a, b in zip(probs, fu.run_harness(harness, probs), fu.run_harness(harness_san, probs)):
        assert a["n_samples"] == b["n_samples"] and np.array_equal(a["seg_first_row"], b["seg_first_row"]), p["name"]
        assert fu.same_bits(a["rows"], b["rows"]) and fu.same_bits(a["grad_waypoints"], b["grad_waypoints"]), p["name"]


class _NoLaunchPlan:
    """a plan's shape without a device: any call that would launch is an error"""
    n_paths, n_segments = 3, 7

    def __getattr__(self, name):
        raise AssertionError("fallback_trajectory reached plan.%s before it had checked its arguments" % name)


def test_fallback_trajectory_checks_every_shape_before_it_launches():
    """a mis-shaped tensor raises ValueError before the unwrap or the clock is launched: those kernels read and write
    [sum V] rows of whatever they are handed"""
    import torch
    from mrs_uav_trajectory_generation_amd import autograd
    plan = _NoLaunchPlan()
    nV = plan.n_segments + plan.n_paths
    wp, lim = torch.zeros((nV, 4), dtype=torch.float64), torch.ones((plan.n_paths, 9), dtype=torch.float64)
    stop, relax = torch.zeros(nV, dtype=torch.uint8), torch.zeros(plan.n_paths, dtype=torch.bool)
    bad = [dict(waypoints=wp[:-1]), dict(waypoints=wp[:, :3]), dict(waypoints=wp.reshape(-1)),
           dict(waypoints=torch.zeros((nV + 1, 4), dtype=torch.float64)), dict(limits=lim[:-1]), dict(limits=lim[:, :8]),
           dict(stop_at=stop[:-1]), dict(stop_at=stop.reshape(-1, 1)), dict(relax_heading=relax[:-1]),
           dict(relax_heading=[True] * (plan.n_paths + 1)), dict(relax_heading=torch.zeros((plan.n_paths, 1), dtype=torch.bool))]
    for kw in bad:
        args = dict(waypoints=wp, limits=lim, stop_at=stop, relax_heading=relax)
        args.update(kw)
        with pytest.raises(ValueError):
            autograd.fallback_trajectory(plan, args["waypoints"], args["limits"], 0.2, 16, stop_at=args["stop_at"],
                                         relax_heading=args["relax_heading"])
    with pytest.raises(AssertionError, match="before it had checked"):     # well-shaped arguments do get as far as the plan
        autograd.fallback_trajectory(plan, wp, lim, 0.2, 16, stop_at=stop, relax_heading=relax)

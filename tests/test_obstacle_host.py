"""The clearance from static obstacles and its backward pass on the CPU: csrc/mrs_tg_obstacle.hpp (the clamped set bounds, the
signed distance, the running minimum, the row gradient of obstacle_clearance_kernel / obstacle_clearance_vjp_kernel) compiled
by g++ into tests/host/obstacle_harness.cpp, against the numpy restatement of tests/obstacle_util.py in BITS (both sides do the
same IEEE operations; sqrt is correctly rounded on both) and against torch's float64 autograd of sqrt(...) - radius gathered at
the forward's nearest obstacles (to 1e-13 of the sum of the absolute terms); the exact zeros of the contract; the defensive
rules on offsets, path_set and nearest arrays that are not well-formed, also in a stand-alone build of the same harness under
AddressSanitizer and UndefinedBehaviorSanitizer, run as its own process; and the Python-side host checks.  No GPU."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from tests import obstacle_util as ou


@pytest.fixture(scope="module")
def cases():
    return ou.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ou.build_harness(tmp_path_factory.mktemp("obstacle"))


@pytest.fixture(scope="module")
def numpy_results(cases):
    """the restatement, once for all tests"""
    return {name: ou.obstacle_clearance_numpy(ou.batch_arrays(c), second=True) for name, c in cases.items()}


def test_cases_have_the_properties_their_names_state(cases, numpy_results):
    res = numpy_results
    for m in ou.ROW_COUNTS:
        assert [p["rows"].shape[0] for p in cases["rows_%d" % m]["paths"]] == [m, m]
        assert np.all(res["rows_%d" % m]["nearest"][:, :m] >= 0) and np.all(res["rows_%d" % m]["nearest"][:, m:] == -1)
    over = cases["count_of_capacity_plus_1"]
    assert all(p["n_samples"] == ou.capacity_of(over) + 1 for p in over["paths"])
    assert np.all(res["count_of_capacity_plus_1"]["nearest"] >= 0)
    r, c = res["dead_path_of_nan_rows_between_live_ones"], cases["dead_path_of_nan_rows_between_live_ones"]
    assert [p["status"] for p in c["paths"]] == [1, 0, 1] and np.isnan(c["paths"][1]["rows"]).all()
    assert np.all(r["nearest"][[0, 2], :12] >= 0) and np.all(r["nearest"][1] == -1) and np.all(np.isinf(r["clearance"][1]))
    for g in ou.SET_SIZES:
        c, r = cases["set_of_%d" % g], res["set_of_%d" % g]
        assert c["sets"] == [g] and c["obstacles"].shape == (g, 4)
        assert np.all(r["nearest"][0, :66] >= 0 if g else r["nearest"] == -1)
        if g:
            assert r["nearest"][1, 0] == g - 1                              # (the last obstacle of the set wins somewhere)
        if g > 8:
            assert len(np.unique(r["nearest"][0, :66])) > 5                 # (the winners are all over the set)
    c, r = cases["sets_3_0_1_5"], res["sets_3_0_1_5"]
    assert c["sets"] == [3, 0, 1, 5] and c["path_set"] == [0, 0, 1, 2, 3, -1, 4]
    n = [p["rows"].shape[0] for p in c["paths"]]
    assert all(np.all((r["nearest"][q, :n[q]] >= 0) & (r["nearest"][q, :n[q]] < 3)) for q in (0, 1))     # two paths share set 0
    assert np.all(r["nearest"][3, :n[3]] == 3) and np.all((r["nearest"][4, :n[4]] >= 4) & (r["nearest"][4, :n[4]] < 9))
    for q in (2, 5, 6):          # the empty set, no set, a set behind the last
        assert np.all(r["nearest"][q] == -1) and np.all(np.isinf(r["clearance"][q])) and np.all(r["argmin"][q] == -1)
    c, r = cases["sets_3_0_1_5_path_set_null"], res["sets_3_0_1_5_path_set_null"]
    assert c["path_set"] is None and ou.batch_arrays(c)["path_set"] is None
    assert np.all(r["nearest"] < 3) and np.all(r["nearest"][0, :40] >= 0)
    # the exact ties: both obstacles at exactly the same c, the lower index wins
    for name, pair in (("exact_tie_lower_index_wins", (0, 1)), ("exact_tie_behind_a_farther_one", (1, 2)),
                       ("exact_tie_64_obstacles_apart", (3, 67)), ("tie_of_a_point_and_a_sphere_point_first", (0, 1)),
                       ("tie_of_a_point_and_a_sphere_sphere_first", (0, 1))):
        c, r = cases[name], res[name]
        rows, ob = c["paths"][0]["rows"], c["obstacles"]
        m = rows.shape[0]
        d = [np.sqrt(((rows[:, :3] - ob[k, :3]) ** 2).sum(axis=1)) - ob[k, 3] for k in pair]
        assert np.array_equal(d[0], d[1]), name
        assert np.all(r["nearest"][0, :m] == pair[0]) and np.array_equal(r["clearance"][0, :m], d[0]), name
        assert np.array_equal(r["second"][0, :m], d[0]), name                # (the runner-up IS at the same c)
        assert d[0][0] in (4.0, 0.5, 2.0), name                              # row 0: a power of two
    assert cases["exact_tie_64_obstacles_apart"]["obstacles"].shape[0] == 70
    for name in ("tie_of_a_point_and_a_sphere_point_first", "tie_of_a_point_and_a_sphere_sphere_first"):
        assert sorted(cases[name]["obstacles"][:2, 3].tolist()) == [0.0, 2.0]
    # the one-ulp near-ties: the gap is really one ulp, and the nearer one wins in either order
    for name in ou.ONE_ULP_CASES:
        r = res[name]
        first, second = r["clearance"][0, 0], r["second"][0, 0]
        assert second == np.nextafter(first, np.inf) and second > first, name
        assert r["nearest"][0, 0] == (0 if name.endswith("first") else 1), name
    assert res["one_ulp_small_nearer_first"]["clearance"][0, 0] < 1.0 < 1.0e6 < res["one_ulp_large_nearer_first"]["clearance"][0, 0]
    r = res["inside_a_sphere"]
    assert np.any(r["clearance"][0, :17] < 0.0) and np.any(r["clearance"][0, :17] > 0.0) and np.all(r["nearest"][0, :17] == 0)
    assert r["min_clearance"][0] < -2.5 and r["argmin"][0, 1] == 0
    r, c = res["row_on_a_centre"], cases["row_on_a_centre"]
    assert np.array_equal(c["paths"][0]["rows"][2, :3], c["obstacles"][1, :3])
    assert r["clearance"][0, 2] == -0.5 and r["nearest"][0, 2] == 1
    assert not cases["radius_0_cloud"]["obstacles"][:, 3].any() and np.all(res["radius_0_cloud"]["clearance"] >= 0.0)
    r, c = res["nan_coordinate_in_an_obstacle"], cases["nan_coordinate_in_an_obstacle"]
    assert np.isnan(c["obstacles"][0]).any() and np.all(r["nearest"][0, :8] == 1) and np.all(np.isfinite(r["clearance"][0, :8]))
    r = res["nan_in_a_row"]
    assert r["nearest"][0, 3] == -1 and np.isinf(r["clearance"][0, 3]) and r["clearance"][0, 3] > 0 and r["nearest"][0, 2] >= 0
    assert r["nearest"][1, 0] == -1 and r["nearest"][1, 1] >= 0 and r["argmin"][1, 0] >= 1
    r, c = res["infinite_radius"], cases["infinite_radius"]
    assert c["obstacles"][0, 3] == -np.inf and c["obstacles"][3, 3] == np.inf
    assert np.all(r["nearest"][0, :9] == 1) and np.all(np.isfinite(r["clearance"][0, :9]))
    assert np.all(r["nearest"][1, :9] == 3) and np.all(r["clearance"][1, :9] == -np.inf) and r["min_clearance"][1] == -np.inf
    assert res["z_scale_1"]["nearest"][0, 0] == 1 and res["z_scale_half"]["nearest"][0, 0] == 0
    assert res["z_scale_1"]["clearance"][0, 0] == 1.0 and res["z_scale_half"]["clearance"][0, 0] == 0.75
    # the random cases: on EVERY row the nearest and the second-nearest obstacle are apart, so no row is left out anywhere
    rows = 0
    for name in ou.RANDOM_CASES:
        r = res[name]
        has = r["nearest"] >= 0
        both = has & np.isfinite(r["second"])
        assert both.sum() == has.sum(), name                 # (every set that is seen has two obstacles or more)
        size = np.maximum(np.abs(r["second"][both]), np.abs(r["clearance"][both]))
        assert np.all((r["second"][both] - r["clearance"][both]) > ou.GAP * size), name
        rows += int(has.sum())
    assert rows > 1000
    assert np.any(res["random_one_set_z_scale_0_3"]["clearance"] < 0.0)     # (some rows are inside a sphere)


def _check_case(name, c, got, want):
    arr = ou.batch_arrays(c)
    P, cap = arr["samples"].shape[:2]
    assert ou.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["nearest"], want["nearest"]), name
    assert ou.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert np.array_equal(got["nearest"] == -1, got["clearance"] == np.inf), name
    grad, scale = ou.obstacle_clearance_torch_grad(arr, want["nearest"])
    assert ou.grads_agree(got["grad"], grad, scale), name
    # exact zeros: column 3, the rows from n on, dead paths, rows without an obstacle, a row on a centre
    assert not got["grad"][:, :, 3].any(), name
    for q in range(P):
        m = ou.live_rows(arr["n"][q], arr["status"][q], cap)
        assert not got["grad"][q, m:].any(), (name, q)
    assert not got["grad"][scale == 0.0].any(), name
    return int((scale[:, :, :3] > 0.0).sum())


def test_harness_is_the_restatement_in_bits_and_torchs_gradient(harness, cases, numpy_results):
    entries = 0
    for name, c in cases.items():
        entries += _check_case(name, c, ou.run_harness(harness, ou.batch_arrays(c)), numpy_results[name])
    assert entries > 10000                   # gradient entries that were held to torch's


def test_the_roots_the_kernel_spares_change_nothing_and_are_most_of_the_work(harness, cases, numpy_results):
    """obsq::cannot_win, the test by which obstacle_clearance_kernel leaves out the square root of an obstacle that cannot
    win: the harness walks every row with it beside the plain loop and exits with code 3 (run_harness fails) if leaving those
    pairs out ever changes a minimum or an index -- on every named case, the one-ulp near-ties in both orders included.  Here:
    what it spares.  Of a near-tie's two members neither, of an exact tie's neither; of a large map most."""
    for name in ou.ONE_ULP_CASES:       # (three obstacles: the two members of the near-tie and one far away)
        assert ou.run_harness(harness, ou.batch_arrays(cases[name]))["spared"].tolist() == [1], name
    for name in ("exact_tie_lower_index_wins", "exact_tie_behind_a_farther_one"):      # six rows, the far one spared on each
        got = ou.run_harness(harness, ou.batch_arrays(cases[name]))["spared"].tolist()
        assert got == ([6] if name.endswith("wins") else [0]), (name, got)              # (in front, the far one IS the minimum)
    assert ou.run_harness(harness, ou.batch_arrays(cases["infinite_radius"]))["spared"].tolist() == [0, 0]
    for name in ou.RANDOM_CASES:
        arr = ou.batch_arrays(cases[name])
        pairs = sum(ou.live_rows(arr["n"][p], arr["status"][p], arr["samples"].shape[1]) * int(np.diff(ou.path_bounds(arr, p))[0])
                    for p in range(arr["samples"].shape[0]))
        spared = int(ou.run_harness(harness, arr)["spared"].sum())
        assert pairs > 10000 and spared > 0.8 * pairs, (name, spared, pairs)


def test_numpy_gradient_restatement_is_the_harness_in_bits(harness, cases, numpy_results):
    """dL/dsamples restated in numpy -- each quotient rounded, then the product -- against the harness bit for bit"""
    for name, c in cases.items():
        arr = ou.batch_arrays(c)
        got = ou.run_harness(harness, arr)["grad"]
        want = np.zeros_like(got)
        kappa = arr["z_scale"]
        for p, r, k in ou._followed(arr, numpy_results[name]["nearest"]):
            g = arr["upstream"][p, r]
            if g == 0.0:
                continue
            row, ob = arr["samples"][p, r], arr["obstacles"][k]
            dx, dy, dz = row[0] - ob[0], row[1] - ob[1], kappa * (row[2] - ob[2])
            s = np.sqrt((dx * dx + dy * dy) + dz * dz)
            if s == 0.0:
                continue
            want[p, r, :3] = g * (dx / s), g * (dy / s), g * ((kappa * dz) / s)
        assert ou.same_bits(got, want), name


def test_exact_zeros_of_the_contract(harness, cases):
    c = cases["row_on_a_centre"]
    arr = ou.batch_arrays(c)
    arr["upstream"][0, :5] = [1.5, -0.75, 2.0, 0.5, -1.0]
    got = ou.run_harness(harness, arr)
    assert got["nearest"][0, 2] == 1 and not got["grad"][0, 2].any()         # s == 0: exactly 0, not 0/0
    assert got["grad"][0, 1].any() and got["grad"][0, 3].any() and np.all(np.isfinite(got["grad"]))
    # a zero upstream gives exactly 0, also on the +inf rows
    for name in ("random_sets", "sets_3_0_1_5", "infinite_radius"):
        a = ou.batch_arrays(cases[name])
        assert not ou.run_harness(harness, dict(a, upstream=np.zeros_like(a["upstream"])))["grad"].any(), name
    # the rows without an obstacle get exactly 0 whatever the upstream is, infinite and NaN upstreams included
    lone = ou.batch_arrays(cases["set_of_0"])
    assert np.count_nonzero(lone["upstream"]) > 50 and not ou.run_harness(harness, lone)["grad"].any()
    wild = lone["upstream"].copy()
    wild[0, ::2], wild[0, 1::2] = np.inf, np.nan
    assert not ou.run_harness(harness, dict(lone, upstream=wild))["grad"].any()
    # a nearest array of -1 gives exactly 0
    arr = ou.batch_arrays(cases["random_sets"])
    assert not ou.run_harness(harness, arr, nearest=np.full(arr["upstream"].shape, -1))["grad"].any()


def _defensive_runs(exe, cases):
    """offsets, path_set and nearest arrays that are not well-formed: the harness (and with it the header's path_obstacles,
    clrq::group_bounds and nearest_in_set) reads nothing outside the arrays -- the sanitizers watch -- and gives exact zeros
    where the contract says so"""
    c = cases["sets_3_0_1_5"]
    arr = ou.batch_arrays(c)
    P, cap = arr["samples"].shape[:2]
    M = arr["obstacles"].shape[0]
    good = ou.run_harness(exe, arr)
    for off in ([-5, 3, 3, 4, 9], [0, 3, 2, 4, 9], [0, 3, 3, 4, 9000], [7, 5, 3, 1, 0], [-2 ** 31, 2 ** 31 - 1, 0, 9, 9],
                [0, 0, 0, 0, 0], [9000, 9000, 9000, 9000, 9000], [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 5]):
        got = ou.run_harness(exe, dict(arr, set_offsets=np.array(off, dtype=np.int64)))
        assert np.all((got["nearest"] >= -1) & (got["nearest"] < M)), off
        assert np.array_equal(got["nearest"] == -1, got["clearance"] == np.inf) and np.all(np.isfinite(got["grad"])), off
    # fewer sets than path_set names, and none at all
    for off in ([0, 9], [4]):
        got = ou.run_harness(exe, dict(arr, set_offsets=np.array(off, dtype=np.int64)))
        names_a_set = (arr["path_set"] >= 0) & (arr["path_set"] < len(off) - 1)
        assert np.all(got["nearest"][~names_a_set] == -1) and np.all((got["nearest"] >= -1) & (got["nearest"] < M))
    # [0, 3, 3, 4, 9000] clamps the last set's end to n_obstacles: the well-formed answer
    got = ou.run_harness(exe, dict(arr, set_offsets=np.array([0, 3, 3, 4, 9000], dtype=np.int64)))
    assert ou.same_bits(got["clearance"], good["clearance"]) and ou.same_bits(got["grad"], good["grad"])
    # path_set out of range: such a path sees nothing
    for bad in (np.full(P, -2 ** 31), np.full(P, 2 ** 31 - 1), np.full(P, 4), np.full(P, -1)):
        got = ou.run_harness(exe, dict(arr, path_set=bad.astype(np.int64)))
        assert np.all(got["nearest"] == -1) and np.all(got["clearance"] == np.inf) and not got["grad"].any()
    # nearest entries: out of range, or an obstacle of somebody else's set -> exactly 0 from them
    for bad in (np.full((P, cap), M), np.full((P, cap), M + 5), np.full((P, cap), -2 ** 31), np.full((P, cap), 2 ** 31 - 1),
                np.full((P, cap), -2)):
        assert not ou.run_harness(exe, arr, nearest=bad)["grad"].any()
    got = ou.run_harness(exe, arr, nearest=np.full((P, cap), 3))      # obstacle 3 is set 2: path 3's own, nobody else's
    assert got["grad"][3, :30].any() and not np.delete(got["grad"], 3, axis=0).any()
    # no obstacles at all, with offsets that claim some
    got = ou.run_harness(exe, dict(arr, obstacles=np.zeros((0, 4))), nearest=np.full((P, cap), 0))
    assert np.all(got["nearest"] == -1) and not got["grad"].any()


def test_defensive_rules(harness, cases):
    _defensive_runs(harness, cases)


def test_harness_is_clean_under_the_sanitizers(tmp_path, cases, numpy_results):
    """the same stand-alone program built with -fsanitize=address,undefined and run as its own process"""
    exe = ou.build_harness(tmp_path, sanitize=True)
    for name in ("rows_65", "set_of_0", "set_of_65", "sets_3_0_1_5", "sets_3_0_1_5_path_set_null", "nan_in_a_row",
                 "infinite_radius", "random_sets"):
        _check_case(name, cases[name], ou.run_harness(exe, ou.batch_arrays(cases[name])), numpy_results[name])
    _defensive_runs(exe, cases)


def test_host_set_offsets_are_checked():
    assert api.check_set_offsets([0, 3, 3, 4, 9], 9).dtype == np.int32
    assert api.check_set_offsets(np.array([0, 2], dtype=np.int64), 2).tolist() == [0, 2]
    assert api.check_set_offsets([0], 0).tolist() == [0] and api.check_set_offsets([0, 0], 0).tolist() == [0, 0]
    for bad in ([1, 9], [0, 3, 2, 9], [0, 3, 8], [0, 3, 10], [], [[0, 9]], [0.0, 9.0], [-1, 9]):
        with pytest.raises(ValueError):
            api.check_set_offsets(bad, 9)


def test_new_names_of_the_python_layer():
    assert api.CAP_OBSTACLE_CLEARANCE == 131072
    assert (api.KERNEL_OBSTACLE_CLEARANCE, api.KERNEL_OBSTACLE_CLEARANCE_VJP) == (37, 38)
    assert {"mrs_tg_plan_obstacle_clearance", "mrs_tg_plan_obstacle_clearance_vjp"} <= set(api.EXPORTED_SYMBOLS)
    for name in ("obstacle_clearance", "obstacle_clearance_vjp"):
        assert callable(getattr(api.Plan, name))

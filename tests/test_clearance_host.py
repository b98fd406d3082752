"""The mutual clearance within groups of paths and its backward pass on the CPU: csrc/mrs_tg_clearance.hpp (group bounds, the
live-row-at-step test, the distance, the running minimum, the two gradient rows of mutual_clearance_kernel /
mutual_clearance_vjp_kernel) compiled by g++ into tests/host/clearance_harness.cpp, against the numpy restatement of
tests/clearance_util.py in BITS (both sides do the same IEEE operations; sqrt is correctly rounded on both) and against torch's
float64 autograd on the forward's partners (to 1e-13 of the sum of the absolute terms); the exact zeros of the contract; the
defensive rules on offsets and partner arrays that are not well-formed, also under AddressSanitizer and
UndefinedBehaviorSanitizer; and the Python-side check of host group offsets.  No GPU."""
import numpy as np
import pytest

from mrs_uav_trajectory_generation_amd import api
from tests import clearance_util as cu


@pytest.fixture(scope="module")
def cases():
    return cu.named_cases()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return cu.build_harness(tmp_path_factory.mktemp("clearance"))


@pytest.fixture(scope="module")
def numpy_results(cases):
    """the restatement, once for all tests"""
    return {name: cu.mutual_clearance_numpy(cu.batch_arrays(c), second=True) for name, c in cases.items()}


def test_cases_have_the_properties_their_names_state(cases, numpy_results):
    res = numpy_results
    for m in cu.ROW_COUNTS:
        assert [p["rows"].shape[0] for p in cases["rows_%d" % m]["paths"]] == [m, m, m]
    over = cases["count_of_capacity_plus_1"]
    assert all(p["n_samples"] == cu.capacity_of(over) + 1 for p in over["paths"])
    assert cases["group_of_0"]["groups"] == [0, 2]
    for g in cu.GROUP_SIZES[1:]:
        assert cases["group_of_%d" % g]["groups"] == [g] and len(cases["group_of_%d" % g]["paths"]) == g
    assert np.all(np.isinf(res["group_of_1"]["clearance"])) and np.all(res["group_of_1"]["partner"] == -1)
    assert cases["groups_3_0_1_5"]["groups"] == [3, 0, 1, 5]
    r = res["groups_3_0_1_5"]
    assert np.all(r["partner"][:3] < 3) and np.all(r["partner"][3] == -1) and np.all((r["partner"][4:] == -1) | (r["partner"][4:] >= 4))
    for k in cu.STEP_OFFSETS:     # the overlap starts at row k of path 0 and ends at row 130 - k of path 1: across the chunk seams
        c, r = cases["offset_%d" % k], res["offset_%d" % k]
        assert [p["first_step"] for p in c["paths"]] == [0, k]
        assert np.all(r["partner"][0, :k] == -1) and np.all(r["partner"][0, k:130] == 1) and np.all(r["partner"][0, 130:] == -1)
        assert np.all(r["partner"][1, :130 - k] == 0) and np.all(r["partner"][1, 130 - k:] == -1)
    assert min(p["first_step"] for p in cases["negative_offset"]["paths"]) < 0
    assert np.any(res["negative_offset"]["partner"] >= 0)
    assert {p["first_step"] for p in cases["extreme_first_steps"]["paths"]} == {2 ** 30, 2 ** 30 - 5, -2 ** 30}
    r = res["extreme_first_steps"]
    assert np.all(r["partner"][0, :61] == 1) and np.all(r["partner"][0, 61:] == -1) and np.all(r["partner"][2] == -1)
    r = res["never_overlap"]
    assert np.all(np.isinf(r["clearance"])) and np.all(r["partner"] == -1) and np.all(r["argmin"] == -1)
    # the exact tie: both neighbours at exactly the same distance, the lower index wins
    for name, subject, want in (("exact_tie_lower_index_wins", 0, 1), ("tie_between_a_path_in_front_and_one_behind", 1, 0)):
        rows = [p["rows"] for p in cases[name]["paths"]]
        others = [q for q in range(3) if q != subject]
        d = [np.sqrt(((rows[subject][:, :3] - rows[q][:, :3]) ** 2).sum(axis=1)) for q in others]
        assert np.array_equal(d[0], d[1]) and np.all(d[0] == 2.0 ** (np.arange(6) - 2.0))
        assert np.all(res[name]["partner"][subject, :6] == want) and want == min(others)
        assert np.array_equal(res[name]["clearance"][subject, :6], d[0])
    assert min(others) < 1 < max(others)          # (the second: one neighbour in front of the subject, one behind it)
    r = res["coincident_rows"]
    assert np.all(r["clearance"][0, 2:5] == 0.0) and np.all(r["clearance"][1, 2:5] == 0.0) and np.all(r["clearance"][0, :2] > 0.0)
    r, c = res["nan_row_in_a_neighbour"], cases["nan_row_in_a_neighbour"]
    assert np.isnan(c["paths"][1]["rows"][5]).any()
    assert np.all(np.delete(r["partner"][0, :12], 5) == 1) and r["partner"][0, 5] == 2 and np.isfinite(r["clearance"][0, 5])
    assert r["partner"][1, 5] == -1 and np.isinf(r["clearance"][1, 5])
    r = res["nan_row_in_the_subject"]
    assert r["partner"][0, 3] == -1 and np.isinf(r["clearance"][0, 3]) and r["partner"][1, 3] == 2 and r["partner"][1, 2] == 0
    r, c = res["dead_path_of_nan_rows_between_live_ones"], cases["dead_path_of_nan_rows_between_live_ones"]
    assert [p["status"] for p in c["paths"]] == [1, 0, 1] and np.isnan(c["paths"][1]["rows"]).all()
    assert np.all(r["partner"][0, :12] == 2) and np.all(r["partner"][1] == -1) and np.all(r["partner"][2, :12] == 0)
    assert np.all(res["z_scale_1"]["partner"][0, :5] == 2) and np.all(res["z_scale_half"]["partner"][0, :5] == 1)
    assert np.all(res["z_scale_1"]["clearance"][0, :5] == 1.0) and np.all(res["z_scale_half"]["clearance"][0, :5] == 0.75)
    r = res["a_row_that_is_partner_to_several_paths"]
    assert np.all(r["partner"][[0, 1, 3, 4], :70] == 2)        # every row of path 2 is the partner of four paths: five terms
    # the random cases: on every row the nearest and the second-nearest neighbour are apart, so no row is left out anywhere
    rows = 0
    for name in cu.RANDOM_CASES:
        r = res[name]
        has = r["partner"] >= 0
        both = has & np.isfinite(r["second"])
        assert np.all((r["second"][both] - r["clearance"][both]) > cu.GAP * r["clearance"][both]), name
        assert np.all(r["clearance"][has] > 1e-3) and both.sum() > 300, name
        assert all(p["rows"][:, :3].min() >= 0.0 and p["rows"][:, :3].max() <= cu.BOX for p in cases[name]["paths"])
        rows += int(has.sum())
    assert rows > 1500


def _check_case(name, c, got, want):
    arr = cu.batch_arrays(c)
    P, cap = arr["samples"].shape[:2]
    assert cu.same_bits(got["clearance"], want["clearance"]), name
    assert np.array_equal(got["partner"], want["partner"]), name
    assert cu.same_bits(got["min_clearance"], want["min_clearance"]) and np.array_equal(got["argmin"], want["argmin"]), name
    assert np.array_equal(got["partner"] == -1, np.isinf(got["clearance"])), name
    grad, scale = cu.mutual_clearance_torch_grad(arr, want["partner"])
    assert cu.grads_agree(got["grad"], grad, scale), name
    # exact zeros: column 3, the rows from n on, dead paths, rows nobody is near, coincident pairs
    assert not got["grad"][:, :, 3].any(), name
    for q in range(P):
        m = cu.live_rows(arr["n"][q], arr["status"][q], cap)
        assert not got["grad"][q, m:].any(), (name, q)
    assert not got["grad"][scale == 0.0].any(), name


def test_harness_is_the_restatement_in_bits_and_torchs_gradient(harness, cases, numpy_results):
    for name, c in cases.items():
        _check_case(name, c, cu.run_harness(harness, cu.batch_arrays(c)), numpy_results[name])


def test_exact_zeros_of_the_contract(harness, cases):
    c = cases["coincident_rows"]
    arr = cu.batch_arrays(c)
    got = cu.run_harness(harness, arr)
    # coincident rows name each other and contribute exactly 0 both ways: rows 2 .. 4 of paths 0 and 1 get only what path 2 gives
    assert np.all(got["partner"][0, 2:5] == 1) and np.all(got["partner"][1, 2:5] == 0)
    names_them = (got["partner"][2, 2:5] == 0) | (got["partner"][2, 2:5] == 1)
    assert names_them.all()
    for r in range(2, 5):
        other = 1 - int(got["partner"][2, r])
        assert not got["grad"][other, r].any()
    # a zero upstream gives exactly 0, also on the +inf rows
    arr0 = dict(arr, upstream=np.zeros_like(arr["upstream"]))
    assert not cu.run_harness(harness, arr0)["grad"].any()
    lone = cu.batch_arrays(cases["never_overlap"])
    assert np.count_nonzero(lone["upstream"]) > 100 and not cu.run_harness(harness, lone)["grad"].any()
    # a partner array of -1 gives exactly 0
    assert not cu.run_harness(harness, arr, partner=np.full(arr["upstream"].shape, -1))["grad"].any()


def _defensive_runs(exe, cases):
    """offsets and partner arrays that are not well-formed: the harness (and with it the header's group_bounds, group_of,
    partner_in_group and row_at_step) reads nothing outside the arrays -- the sanitizers watch -- and gives exact zeros where
    the contract says so"""
    c = cases["groups_3_0_1_5"]
    arr = cu.batch_arrays(c)
    P, cap = arr["samples"].shape[:2]
    good = cu.run_harness(exe, arr)
    for off in ([-5, 3, 3, 4, 9], [0, 3, 2, 4, 9], [0, 3, 3, 4, 9000], [7, 5, 3, 1, 0], [-2 ** 31, 2 ** 31 - 1], [0, 0], [4]):
        got = cu.run_harness(exe, dict(arr, group_offsets=np.array(off, dtype=np.int64)))
        assert np.all((got["partner"] >= -1) & (got["partner"] < P))
        assert np.array_equal(got["partner"] == -1, np.isinf(got["clearance"])) and np.all(np.isfinite(got["grad"]))
    # [0, 3, 3, 4, 9000] clamps the last group's end to n_paths: the well-formed answer
    got = cu.run_harness(exe, dict(arr, group_offsets=np.array([0, 3, 3, 4, 9000], dtype=np.int64)))
    assert cu.same_bits(got["clearance"], good["clearance"]) and cu.same_bits(got["grad"], good["grad"])
    # partner entries: out of range, out of group, the row's own path, a path without a row at the step -> exactly 0 from them
    own = np.repeat(np.arange(P, dtype=np.int64)[:, None], cap, axis=1)
    for bad in (np.full((P, cap), P + 5), np.full((P, cap), -2 ** 31), np.full((P, cap), 2 ** 31 - 1), own,
                np.full((P, cap), 3)):       # (path 3 is a group of its own: out of group for everyone else, own path for itself)
        assert not cu.run_harness(exe, arr, partner=bad)["grad"].any()
    late = cu.batch_arrays(cases["offset_65"])
    names_absent = np.array([np.full(late["upstream"].shape[1], 1), np.full(late["upstream"].shape[1], 0)])
    got = cu.run_harness(exe, late, partner=names_absent)
    assert not got["grad"][0, :65].any() and got["grad"][0, 65:130].any()     # rows 0 .. 64 of path 0: path 1 has no row there
    assert not got["grad"][1, 65:].any()


def test_defensive_rules(harness, cases):
    _defensive_runs(harness, cases)


def test_harness_is_clean_under_the_sanitizers(tmp_path, cases, numpy_results):
    exe = cu.build_harness(tmp_path, sanitize=True)
    for name in ("rows_65", "groups_3_0_1_5", "offset_64", "extreme_first_steps", "nan_row_in_a_neighbour", "random_groups"):
        _check_case(name, cases[name], cu.run_harness(exe, cu.batch_arrays(cases[name])), numpy_results[name])
    _defensive_runs(exe, cases)


def test_host_group_offsets_are_checked():
    assert api.check_group_offsets([0, 3, 3, 4, 9], 9).dtype == np.int32
    assert api.check_group_offsets(np.array([0, 2], dtype=np.int64), 2).tolist() == [0, 2]
    for bad in ([1, 9], [0, 3, 2, 9], [0, 3, 8], [0, 3, 10], [], [[0, 9]], [0.0, 9.0], [-1, 9]):
        with pytest.raises(ValueError):
            api.check_group_offsets(bad, 9)

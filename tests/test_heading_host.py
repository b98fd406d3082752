"""The heading along the direction of travel and its backward pass on the CPU: csrc/mrs_tg_heading.hpp (the step, the source
test, the heading and the gradient rows of travel_heading_kernel / travel_heading_vjp_kernel) compiled by g++ into
tests/host/heading_harness.cpp, against the numpy restatement of the reference's loop (sources and headings exactly: both sides
use libm) and against torch's autograd on the fixed sources (gradients to 1e-13 of the sum of the absolute terms).  No GPU."""
import math

import numpy as np
import pytest

from tests import heading_util as hu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return hu.build_harness(tmp_path_factory.mktemp("heading"))


def _check_batch(name, batch, res):
    samples, n, status, upstream = hu.batch_arrays(batch)
    cap = samples.shape[1]
    for q, r in enumerate(res):
        m = hu.live_rows(n[q], status[q], cap)
        assert r["m"] == m, (name, q)
        heading, source = hu.travel_heading_numpy(samples[q, :m], atan2=math.atan2)   # libm on both sides
        assert np.array_equal(r["source"], source), (name, q)
        assert np.array_equal(hu.travel_heading_numpy(samples[q, :m])[1], source), (name, q)
        assert hu.same_bits(r["heading"], heading), (name, q)
        want = hu.travel_heading_torch_grad(samples[q, :m], upstream[q, :m], source)
        assert hu.grads_agree(r["grad"], want, hu.grad_scale(samples[q, :m], upstream[q, :m], source)), (name, q)
        # what passes through passes through exactly
        assert hu.same_bits(r["grad"][:, 2], upstream[q, :m, 2]), (name, q)
        if m:
            assert hu.same_bits(r["grad"][m - 1, 3], upstream[q, m - 1, 3]) and not r["grad"][:m - 1, 3].any(), (name, q)


def test_cases_have_the_properties_their_names_state():
    cases = hu.named_cases()
    src = {name: [hu.travel_heading_numpy(p["rows"])[1] for p in batch] for name, batch in cases.items()}
    hdg = {name: [hu.travel_heading_numpy(p["rows"])[0] for p in batch] for name, batch in cases.items()}
    for n in (0, 1, 2, 3, 64, 65, 128, 129, 130):
        assert cases["n%d" % n][0]["rows"].shape[0] == n
    s = src["slow_run_62_to_66"][0]
    assert s[61] == 61 and set(s[62:67]) == {61} and s[67] == 67
    s = src["slow_run_of_70_rows"][0]
    assert set(s[60:130]) == {59} and s[130] == 130
    s = src["slow_from_row_1_to_the_end"][0]
    assert set(s[:149]) == {0} and s[149] == -1
    s, h = src["zero_step_at_row_0_then_slow"][0], hdg["zero_step_at_row_0_then_slow"][0]
    assert set(s[:-1]) == {0} and not h[:-1].any()
    s = src["every_step_a_source"][0]
    assert np.array_equal(s[:-1], np.arange(129))
    s, h = src["step_of_exactly_the_threshold"][0], hdg["step_of_exactly_the_threshold"][0]
    rows = cases["step_of_exactly_the_threshold"][0]["rows"]
    assert rows[2, 0] - rows[1, 0] == 0.05 and s.tolist() == [0, 1, 1, 3, -1] and h[1] == 0.0 and h[0] != 0.0
    h = hdg["negative_zero_dy_is_minus_pi"][0]
    assert h[:4].tolist() == [-math.pi, math.pi, -math.pi, math.pi]
    over = cases["count_of_capacity_plus_1"]
    assert over[0]["n_samples"] == hu.capacity_of(over) + 1
    assert [p["status"] for p in cases["dead_path_between_live_ones"]] == [1, 0, 1]
    s, h = src["not_a_number_in_a_middle_row"][0], hdg["not_a_number_in_a_middle_row"][0]
    assert np.isnan(h[39:51]).all() and np.isfinite(h[:39]).all() and np.isfinite(h[51:]).all() and set(s[40:51]) == {40}
    assert sorted({p["rows"].shape[0] for p in cases["five_paths"]}) == [3, 65, 100, 130, 200]
    # every step's length is one of the stated ones, none within 1e-3 of the threshold (the exact-threshold case apart), and the
    # directions cover the four quadrants and the axes
    seen = set()
    for name, batch in cases.items():
        for p in batch:
            r = p["rows"]
            dd = r[1:, :2] - r[:-1, :2]
            dd = dd[np.isfinite(dd).all(axis=1)]
            d = np.hypot(dd[:, 0], dd[:, 1])
            if name not in ("step_of_exactly_the_threshold", "negative_zero_dy_is_minus_pi"):
                assert np.all(np.min(np.abs(d[:, None] - np.array(hu.STEP_LENGTHS)[None, :]), axis=1) < 1e-12), name
            if name != "step_of_exactly_the_threshold":
                assert np.all(np.abs(d - hu.MIN_STEP) >= 1e-3 - 1e-12), name
            seen |= {(int(np.sign(round(x, 9))), int(np.sign(round(y, 9)))) for x, y in dd}
    assert {(1, 1), (-1, 1), (-1, -1), (1, -1), (1, 0), (-1, 0), (0, 1), (0, -1), (0, 0)} <= seen


def test_harness_is_the_reference_loop_and_its_gradient(harness):
    for name, batch in hu.named_cases().items():
        _check_batch(name, batch, hu.run_harness(harness, batch))


def test_harness_is_clean_under_the_sanitizers(tmp_path):
    exe = hu.build_harness(tmp_path, sanitize=True)
    for name, batch in hu.named_cases().items():
        _check_batch(name, batch, hu.run_harness(exe, batch))

"""The C oracle against the 60-digit ground-truth fixtures (tests/golden, made by oracle/gen_golden.py).

The oracle follows the reference's arithmetic route, whose own error is what these bounds record
(SURVEY.md 8c measured 5e-12 .. 2e-10 for T in [0.05, 20] s with snap; acceleration cost and very short
segments are worse).  The bounds are per-case ceilings with head-room, not targets.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import util


def _tol_coeff(case):
    if case["name"] == "bench_slot15_path237_short_segment":
        # the worst-conditioned of the 20 480 paths the headline's timed region solves (a 0.179 s segment between 4.7 s and
        # 4.0 s ones): the reference-style double route is 5.4e-7 off the 60-digit solution HERE -- the figure bench.py reports
        # as in_flight_slots_vs_cpu_ref.max_coeff_err_vs_cpu_ref is this oracle's error (the HIP path: ~2e-9,
        # tests/test_gpu_headline_kernel.py)
        return 1e-6
    if "short" in case["name"]:
        return 2e-7
    return {2: 5e-8, 3: 1e-9, 4: 1e-9}[case["derivative_to_optimize"]]


def test_oracle_coefficients_and_cost(golden):
    assert len(golden["cases"]) >= 10
    for case in golden["cases"]:
        d, m, v, t, _ = util.case_arrays(case)
        c = po.solve_linear(d, m, v, t)
        exact = np.array(case["coeffs"])
        assert util.coeff_error(c, exact) < _tol_coeff(case), case["name"]
        if case["name"] == "bench_slot15_path237_short_segment":
            assert util.coeff_error(c, exact) > 2e-7   # asserted, not narrated: the double oracle is the inaccurate side
        J = po.compute_cost(d, t, c)
        assert abs(J - case["cost"]) <= (1e-8 if "slot15" in case["name"] else 1e-9) * abs(case["cost"]), case["name"]


def test_oracle_segment_blocks(golden):
    for case in golden["cases"]:
        if "H" not in case:
            continue
        d, _, _, t, _ = util.case_arrays(case)
        for s, T in enumerate(t):
            H, Ai = po.segment_hessian(d, T)
            He, Ae = np.array(case["H"][s]), np.array(case["Ainv"][s])
            assert np.max(np.abs(H - He)) <= 2e-7 * np.max(np.abs(He)), (case["name"], s)
            assert np.max(np.abs(Ai - Ae)) <= 2e-7 * np.max(np.abs(Ae)), (case["name"], s)


def test_oracle_mellinger_gradient(golden):
    n = 0
    for case in golden["cases"]:
        if "gradient" not in case:
            continue
        n += 1
        d, m, v, t, _ = util.case_arrays(case)
        J, g = po.cost_and_gradient(d, m, v, t)
        ge = np.array(case["gradient"])
        assert abs(J - case["cost"]) <= 1e-9 * abs(case["cost"])
        # forward difference of two ~1e-10-accurate costs over h = 0.1
        assert np.max(np.abs(g - ge)) <= 1e-6 * np.max(np.abs(ge)), case["name"]
    assert n >= 4


def test_survey_probe_values_config1(golden):
    # config 1 with Euclidean times [5, 7.0711, 5]: J_d = 20.4602, grad = [-2.2572, 5.6827, -2.2572]
    case = next(c for c in golden["cases"] if c["name"] == "config1_snap")
    assert abs(case["cost"] - 20.4602) < 1e-4
    assert np.allclose(case["gradient"], [-2.2572, 5.6827, -2.2572], atol=1e-4)


def test_oracle_maxima(golden):
    groups = [[0, 1], [2], [3]]
    n = 0
    for case in golden["cases"]:
        if "maxima" not in case:
            continue
        n += 1
        d, m, v, t, _ = util.case_arrays(case)
        exact_c = np.array(case["coeffs"])
        mx = np.array(case["maxima"])
        for s in range(len(t)):
            for k in (1, 2, 3):
                for gi, grp in enumerate(groups):
                    val = po.segment_max_magnitude(exact_c[s], t[s], k, grp)
                    assert abs(val - mx[s, k - 1, gi]) <= 1e-10 * max(mx[s, k - 1, gi], 1e-6), (case["name"], s, k, gi)
    assert n >= 2


# ---- the oracle's other arithmetic routes (mrs_tg_oracle.h: mto_set_arithmetic) -------------------------------------
# 1: per-segment matrices from exactly rounded unit-time tables; 2: the whole linear solve in 113-bit arithmetic.  Same
# algorithm as route 0 (the reference's), less and less rounding noise; the fixtures are the 60-digit ground truth.

def test_unit_time_tables_equal_the_products_constants():
    """two independent derivations of the same exact rational tables -- mpmath (tools/gen_constants.py -> mrs_tg_constants.h,
    what the kernels use) and __float128 Gauss-Jordan (oracle/mto_linear.c) -- agree to the last bit"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mrs_uav_trajectory_generation_amd", "csrc",
                            "mrs_tg_constants.h")).read()

    def table(name):
        body = re.search(r"#define %s \{(.*?)\n\}\n" % name, src, re.S).group(1)
        return np.array([float.fromhex(t) if "x" in t else float(t)
                         for t in re.findall(r"-?0x[0-9a-f.]+p[+-]?\d+|-?\d+\.\d+", body)])

    a, h = po.unit_tables()
    assert np.array_equal(table("MRS_TG_ABAR_INV_INIT").reshape(10, 10), a)
    assert np.array_equal(table("MRS_TG_HBAR_INIT").reshape(5, 10, 10), h)


def test_unit_time_hessian_is_exactly_time_reversal_symmetric():
    """Reversing a segment's time maps end-point derivative r to (-1)^r times the other end's, and the cost does not change:
    HBAR = P^T HBAR P with P = [[0, D], [D, 0]], D = diag((-1)^r).  The rounded constants keep that symmetry to the last
    bit, which is what would let the lean outer-loop kernels run their right-to-left half sweeps on the LEFT-to-right table in
    sign-transformed variables (the one-table build of profiles/round5_lean_table_ab.txt) and still produce the bits of the mirrored
    table: every entry the right-to-left table of stage_ps_tables holds is the left-to-right entry times sigma_r sigma_c."""
    _, h = po.unit_tables()
    sig = np.array([(-1.0) ** r for r in range(5)])
    for d in range(5):
        H = h[d]
        ss, se, es, ee = H[:5, :5], H[:5, 5:], H[5:, :5], H[5:, 5:]
        assert np.array_equal(ee, ss * np.outer(sig, sig))          # far block  = sigma_r sigma_c x near block
        assert np.array_equal(es, se * np.outer(sig, sig))          # coupling, mirrored (= its transpose by symmetry of H)
        assert np.array_equal(se, se.T * np.outer(sig, sig))
        if d >= 1:   # (order 0 penalises the position itself)
            assert np.array_equal(H[:, 5], -H[:, 0])                # a constant polynomial costs nothing
            assert np.array_equal(H[5:, 0], -sig * H[:5, 0])        # position brackets: end rows from start rows


def test_oracle_routes_against_the_ground_truth(golden):
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    for case in golden["cases"]:
        d, m, v, t, _ = util.case_arrays(case)
        exact = np.array(case["coeffs"])
        for mode in (po.REFERENCE_ARITHMETIC, po.EXACT_CONSTANTS, po.QUAD_PRECISION):
            with po.arithmetic(mode):
                c = po.solve_linear(d, m, v, t)
                J = po.compute_cost(d, t, c)
            e = util.coeff_error(c, exact)
            worst[mode] = max(worst[mode], e)
            if mode == po.QUAD_PRECISION:  # the correctly rounded result
                assert e < 1e-15, (case["name"], e)
                assert abs(J - case["cost"]) <= 4e-16 * abs(case["cost"]), case["name"]
            elif mode == po.EXACT_CONSTANTS and "short" not in case["name"] and "walk" not in case["name"]:
                assert e < 1e-12, (case["name"], e)   # what is left is the dense QR on R_pp in unscaled unknowns
    assert po.lib().mto_get_arithmetic() == 0
    assert worst[2] < worst[1] <= 1e-6 and worst[0] <= 1e-6   # (1e-7 without bench_slot15_path237_short_segment)


def test_quad_route_gradient_and_outer_loop(golden):
    """the outer loop runs on the 113-bit solve as on the others (same stopping reasons on the fixture paths; times within the
    noise the reference-style gradient carries)"""
    n = 0
    for case in golden["cases"]:
        if "gradient" not in case:
            continue
        d, m, v, t, _ = util.case_arrays(case)
        with po.arithmetic(po.QUAD_PRECISION):
            J, g = po.cost_and_gradient(d, m, v, t)
            st2, t2, _, _ = po.optimize_times(d, m, v, t)
        ge = np.array(case["gradient"])
        assert abs(J - case["cost"]) <= 4e-16 * abs(case["cost"])
        assert np.max(np.abs(g - ge)) <= 1e-12 * np.max(np.abs(ge)), case["name"]   # (J' - J) / h of two exact costs
        st0, t0, _, _ = po.optimize_times(d, m, v, t)
        assert st0 == st2 and np.max(np.abs(t0 - t2) / t2) < 1e-4, case["name"]
        n += 1
    assert n >= 4

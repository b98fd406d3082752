"""What the tests of the Baca segment-time estimate as a plan step share (tests/test_baca_host.py, tests/test_gpu_baca.py,
tests/golden/gen_baca_cases.py): the fixture, the harness's line grammar, the tolerances of the issue, the batches and the
restatement of the length gate."""
import os

import numpy as np

from tests import estimate_util as eu
from tests import host_harness as hh

FIXTURES = os.path.join(hh.GOLDEN, "baca_cases.json")
HARNESS = "baca_harness.cpp"
V_VERTICAL, A_VERTICAL, J_VERTICAL, T1_CAPPED, T2_CAPPED, DOT1_CLAMPED, DOT2_CLAMPED = 1, 2, 4, 8, 16, 32, 64
FLOOR, HEADING, HEADING_CRUISE, HEADING_ACC = 128, 256, 512, 1024
ACCEPTED, REJECTED_CODE, TOO_LONG, TOO_SHORT = 0, 1, 2, 3
FLT_MAX = eu.FLT_MAX
# the tolerances of the Baca estimate's tests, derived, not measured:
VALUE_RTOL = eu.VALUE_RTOL          # 1e-13: the project's figure for this estimator family
# Gradient entries: |got - exact| <= K 2^-53 sum|addends| (+ the wrap term on heading entries), K = 10 x the roundings on the
# longest chain of csrc/mrs_tg_baca.hpp -- 25 of them, counted in tests/golden/gen_baca_cases.py
CHAIN_ROUNDINGS = 25
GRAD_RTOL = 10 * CHAIN_ROUNDINGS * 2.0 ** -53
WRAP_ERROR = eu.WRAP_ERROR          # the forward's wrap error in ang: four roundings at magnitude 2 pi
FIXTURE_ERROR = 1e-30               # what the central differences themselves are known to: the generator asserts them
#                                     against the closed forms to 1e-30 (1 + sum|addends|); an entry without addends is 1e-41, not 0
MARGIN = 1e-9                       # the least relative margin to a branch boundary on the GPU tier's batches

bits, same_bits, dyadic, pack, shapes, batch_problems, problem = (eu.bits, eu.same_bits, eu.dyadic, eu.pack, eu.shapes,
                                                                 eu.batch_problems, eu.problem)


def load_cases():
    return hh.load_cases("baca_cases.json")


def build_harness(tmp_path, sanitize=False):
    return hh.build(HARNESS, tmp_path, sanitize=sanitize)


def case_problem(c):
    return problem(c["waypoints"], c["limits"], c["upstream"])


def run_harness(exe, problems, env=None):
    """-> per problem dict(flags [S] int, value [S], margin [S], grad_waypoints [S + 1][4], grad_limits [9], raw)"""
    lines = ["%d %s %s %s\n" % (p["waypoints"].shape[0] - 1, hh.fmt(p["waypoints"]), hh.fmt(p["limits"]), hh.fmt(p["upstream"]))
             for p in problems]
    out = hh.run(exe, lines, len(problems), env=env)
    res = []
    for p, line in zip(problems, out):
        S = p["waypoints"].shape[0] - 1
        x = line.split()
        assert len(x) == 3 * S + 4 * (S + 1) + 9, (len(x), S)
        head = np.array([float(v) for v in x[:3 * S]]).reshape(S, 3)
        rest = np.array([float(v) for v in x[3 * S:]])
        res.append(dict(flags=head[:, 0].astype(np.int64), value=head[:, 1].copy(), margin=head[:, 2].copy(),
                        grad_waypoints=rest[:4 * (S + 1)].reshape(S + 1, 4), grad_limits=rest[4 * (S + 1):].copy(), raw=line))
    return res


def run_gate_harness(exe, gates, env=None):
    """gates: dicts(seg_times, n_samples, dt, max_factor, min_factor, status or None) -> [(total, verdict)]"""
    lines = ["%d %s %d %r %r %r %d %d\n" % (-len(g["seg_times"]), hh.fmt(g["seg_times"]), g["n_samples"], float(g["dt"]),
                                             float(g["max_factor"]), float(g["min_factor"]), int(g["status"] is not None),
                                             0 if g["status"] is None else g["status"]) for g in gates]
    out = hh.run(exe, lines, len(gates), env=env)
    return [(float(line.split()[0]), int(line.split()[1])) for line in out]


def gate_restatement(seg_times, n_samples, dt, max_factor, min_factor, status=None):
    """baca_total_time's sum (csrc/mrs_tg_policy_host.hpp) + code_accepted + length_check (csrc/mrs_tg_baca.hpp) in Python floats (IEEE doubles,
    nothing fused) -> (total, verdict)"""
    total = 0.0
    for t in np.asarray(seg_times, dtype=np.float64):
        total = total + float(t)
    if status is not None and not ((status >= 1 and status != 6) or status == -1):
        return total, REJECTED_CODE
    length = float(n_samples) * float(dt)
    if not length > 1.0:
        return total, ACCEPTED
    if max_factor > 0 and length > max_factor * total:
        return total, TOO_LONG
    if min_factor > 0 and length < min_factor * total:
        return total, TOO_SHORT
    return total, ACCEPTED


def gradient_excess(case, grad_waypoints, grad_limits):
    """the issue's bound per entry, |got - exact| <= K 2^-53 sum|addends|, plus 1.5 * 4e-15 / w^2 on the entries the wrapped
    heading difference enters (the heading column of the waypoints, limits 2 and 5; w the path's heading-rate limit; it
    vanishes for a relaxed heading) and the fixture's own 1e-30 (1 + sum|addends|) -> the largest |error| - bound over the waypoint entries and over the limit entries
    (<= 0: within), and the largest |error| / bound"""
    w = float(case["limits"][2])
    wrap = 1.5 * WRAP_ERROR / (w * w)
    ew = np.abs(np.asarray(grad_waypoints) - np.array(case["grad_waypoints"]))
    el = np.abs(np.asarray(grad_limits) - np.array(case["grad_limits"]))
    bw = GRAD_RTOL * np.array(case["scale_waypoints"]) + FIXTURE_ERROR * (1 + np.array(case["scale_waypoints"]))
    bw[:, 3] += wrap
    bl = GRAD_RTOL * np.array(case["scale_limits"]) + FIXTURE_ERROR * (1 + np.array(case["scale_limits"]))
    bl[[2, 5]] += wrap
    ratio = max(float(np.max(ew / np.maximum(bw, 1e-300) * (ew > 0))), float(np.max(el / np.maximum(bl, 1e-300) * (el > 0))))
    return float(np.max(ew - bw)), float(np.max(el - bl)), ratio
